// k_cabac.hip -- CABAC bit estimator for residual coding: the first building block of SURVEY 8(a) row a0 / 8(f)-1
// (it supplies the rate terms of rows a8, a8b and the tables of a11).
// Replaces: ContextModel::init (TLibCommon/ContextModel.cpp:56-65) with the fork's initialisation tables
// (TLibCommon/ContextTables.h:340-546, five slice types), the state transition / fractional bit tables (:67-128,
// FAST_BIT_EST), TEncSbac::estBit (TLibEncoder/TEncSbac.cpp:2175-2370) and -- on the device, for batches of TUs --
// TEncSbac::codeCoeffNxN (:1829-2092) + codeLastSignificantXY (:1772-1827) + codeTransformSkipFlags (:1608-1628) +
// xWriteCoefRemainExGolomb (:381-402) driven through the counting bin coder (TEncBinCoderCABACCounter.cpp:72-108).
//
// Mapping: the coder is a serial walk with adaptive context states, so ONE LANE codes one TU (64 TUs per wave); the
// 150 context states of each lane live in LDS ([state][lane] bytes), the 64-bit coefficient-group map in a register
// pair.  Every TU starts from the context snapshot its job names -- the RD search of the reference loads a snapshot
// before every test (TEncSbac::load, m_pppcRDSbacCoder) -- and can hand back the updated states.
#include <string.h>
#include "hop_dev.h"
#include "hop_cabac_tab.h"

__constant__ uint8_t c_next_mps[128] = HOP_NEXT_MPS;
__constant__ uint8_t c_next_lps[128] = HOP_NEXT_LPS;
__constant__ int32_t c_entropy_bits[128] = HOP_ENTROPY_BITS;
static const int32_t h_entropy_bits[128] = HOP_ENTROPY_BITS;
// the three tables above packed for the one-lane coders (hop_cabac_tab.h), and the copy of it a workgroup keeps in LDS: ONE table per workgroup, a variable of its own at
// file scope -- outside every union (WalkShared's halves overwrite each other), and every function reaches it by name, also where the compiler makes a coder body a
// function of its own: the address space is the variable's, so the bin is a ds_read_b32.  Only the kernels that code bins on CabacLds1 hold it (1 KB of LDS each).
__constant__ hop_bin_table c_bin_table = hop_make_bin_table();
__shared__ uint32_t s_bin_table[256];

// offsets of the context sets inside hop_cabac_ctx.state (the reference's set order, TEncSbac.cpp:76-88)
#define CX_QT_CBF 0
#define CX_TRANS_SUBDIV 8
#define CX_ROOT_CBF 11
#define CX_SIG_CG 12
#define CX_SIG 16
#define CX_LAST_X 58
#define CX_LAST_Y 88
#define CX_ONE 118
#define CX_ABS 142
#define CX_TS 148
#define CX_COUNT 150

// (context initialisation and TEncSbac::estBit are host logic: host/hop_hostlogic.cpp)

// ---- device: counted bits of codeCoeffNxN, one lane per TU ----
struct CabacLds { uint8_t st[172][64]; uint16_t absCoeff[16][64]; };      // rows 0..151: hop_cabac_ctx; 152..171: the CU-level sets of hop_cabac_cu_ctx (k_rqt.inl)

struct CabacLds1 { uint8_t st[172][1]; uint16_t absCoeff[16][1]; };         // the same for ONE lane (a TU or CU with a wave of its own): 204 bytes instead of 13 KB

// One context-coded bin: the bits of bin b in state s added to frac, the next state returned.  The form is picked by the type of the coder's states:
//   CabacLds   64 lanes side by side: the __constant__ tables (64 lanes share each round trip);
//   CabacLds1  one working lane: the workgroup's packed table in LDS, one ds_read_b32 -- the kernel has filled it at its entry (cab_bin_fill).
__device__ static __forceinline__ uint8_t cab_bin(const CabacLds&, const uint8_t s, const int b, unsigned long long& frac) {
  frac += (unsigned long long)c_entropy_bits[s ^ b];
  return ((s & 1) == b) ? c_next_mps[s] : c_next_lps[s];
}
__device__ static __forceinline__ uint8_t cab_bin(const CabacLds1&, const uint8_t s, const int b, unsigned long long& frac) {
  const uint32_t e = s_bin_table[((unsigned)s << 1) | (unsigned)b];
  frac += (unsigned long long)HOP_BIN_BITS(e);
  return (uint8_t)HOP_BIN_NEXT(e);
}
#define CBIN(idx, b) do { const int i_ = (idx); const uint8_t s_ = sh.st[i_][lane]; sh.st[i_][lane] = cab_bin(sh, s_, (b), frac); } while (0)

// The workgroup's copy of the packed table, by ALL its threads at the kernel's entry: every thread of the workgroup calls this before anything else (before any early
// return, outside any `if (live)` / `if (tid == 0)`) -- the barrier is inside.  Nothing writes the table afterwards.
__device__ static __forceinline__ void cab_bin_fill() {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_bin_table[i] = c_bin_table.v[i];
  __syncthreads();
}
// The candidate walks (k_walk.inl) keep the scan tables (hop_rdoq_build_scans: 3 x 1360 + 3 x 85 entries, 8 670 bytes) in LDS beside it, in the device table's layout: the
// node coders and the CU-level counters read scan[pos] and then coef[scan[pos]] for every position at or below the last one -- the first of the two dependent loads then
// is no HBM load -- and a leaf's per-unit copy of its scan reads from here.  Same rules as cab_bin_fill, which this includes: all threads, the kernel's entry, one barrier.
__shared__ __attribute__((aligned(4))) uint16_t s_scan_tables[HOP_RDOQ_SCAN_ENTRIES + 1];
__device__ static __forceinline__ void walk_tables_fill(const uint16_t* __restrict__ scans) {
  const uint32_t* s32 = (const uint32_t*)scans; uint32_t* d32 = (uint32_t*)s_scan_tables;   // (the device table is hipMalloc'ed: aligned; an odd number of entries)
  for (int i = threadIdx.x; i < HOP_RDOQ_SCAN_ENTRIES / 2; i += blockDim.x) d32[i] = s32[i];
  if (threadIdx.x == 0) s_scan_tables[HOP_RDOQ_SCAN_ENTRIES - 1] = scans[HOP_RDOQ_SCAN_ENTRIES - 1];
  cab_bin_fill();
}
template <class LDS> __device__ static __forceinline__ void cab_bin_fill_for();          // (the kernels that are templates over the coder's form)
template <> __device__ __forceinline__ void cab_bin_fill_for<CabacLds>() {}
template <> __device__ __forceinline__ void cab_bin_fill_for<CabacLds1>() { cab_bin_fill(); }

// counted bits of one TU on the lane's context states: the coded_block_flag if asked for (encodeQtCbf), then codeCoeffNxN
template <class LDS>
__device__ static unsigned long long cb_code_tu_at(LDS& sh, const int lane, const int32_t* __restrict__ coef, const int log2, const int chroma, const int scan_idx,
                                                   const int sign_hide, const int use_ts, const int ts_flag, const int cbf_ctx_plus1,
                                                   const uint16_t* __restrict__ scan, const uint16_t* __restrict__ scanCG);
template <class LDS>
__device__ static unsigned long long cb_code_tu(LDS& sh, const int lane, const int32_t* __restrict__ coef, const int log2, const int chroma, const int scan_idx,
                                                const int sign_hide, const int use_ts, const int ts_flag, const int cbf_ctx_plus1, const uint16_t* __restrict__ scans) {
  const int so = (log2 == 2) ? 0 : (log2 == 3) ? 16 : (log2 == 4) ? 80 : 336, co = (log2 == 2) ? 0 : (log2 == 3) ? 1 : (log2 == 4) ? 5 : 21;
  return cb_code_tu_at(sh, lane, coef, log2, chroma, scan_idx, sign_hide, use_ts, ts_flag, cbf_ctx_plus1, scans + scan_idx * 1360 + so, scans + 4080 + scan_idx * 85 + co);
}
// the same with the TU's scan and coefficient-group scan given (a caller that holds them in LDS)
template <class LDS>
__device__ static unsigned long long cb_code_tu_at(LDS& sh, const int lane, const int32_t* __restrict__ coef, const int log2, const int chroma, const int scan_idx,
                                                   const int sign_hide, const int use_ts, const int ts_flag, const int cbf_ctx_plus1,
                                                   const uint16_t* __restrict__ scan, const uint16_t* __restrict__ scanCG) {
  unsigned long long frac = 0;
  const int width = 1 << log2, nco = width * width;
  int numSig = 0;
  for (int i = 0; i < nco; i++) numSig += coef[i] != 0;
  if (cbf_ctx_plus1) CBIN(CX_QT_CBF + cbf_ctx_plus1 - 1, numSig != 0 ? 1 : 0);      // encodeQtCbf (TEncSbac.cpp:1596-1600)
  if (numSig != 0) {
    if (use_ts && width == 4) CBIN(CX_TS + chroma, ts_flag ? 1 : 0);
    unsigned long long cgFlag = 0;
    const int numBlkSide = width >> 2;
    int scanPosLast = -1, posLast;
    do {
      posLast = scan[++scanPosLast];
      const int py = posLast >> log2, px = posLast - (py << log2);
      const int c = coef[posLast];
      if (c) cgFlag |= 1ull << (numBlkSide * (py >> 2) + (px >> 2));
      numSig -= (c != 0);
    } while (numSig > 0);
    {                                                            // codeLastSignificantXY
      int posY = posLast >> log2, posX = posLast - (posY << log2);
      if (scan_idx == 2) { const int t = posX; posX = posY; posY = t; }
      const int gX = hop_group_idx(posX), gY = hop_group_idx(posY), gMax = hop_group_idx(width - 1);
      const int cb = log2 - 2;
      const int off = chroma ? 0 : (cb * 3 + ((cb + 1) >> 2)), shf = chroma ? cb : ((cb + 3) >> 2);
      const int bx = CX_LAST_X + 15 * chroma + off, by = CX_LAST_Y + 15 * chroma + off;
      int k;
      for (k = 0; k < gX; k++) CBIN(bx + (k >> shf), 1);
      if (gX < gMax) CBIN(bx + (k >> shf), 0);
      for (k = 0; k < gY; k++) CBIN(by + (k >> shf), 1);
      if (gY < gMax) CBIN(by + (k >> shf), 0);
      if (gX > 3) frac += 32768ull * (unsigned long long)((gX - 2) >> 1);
      if (gY > 3) frac += 32768ull * (unsigned long long)((gY - 2) >> 1);
    }
    const int baseCG = CX_SIG_CG + 2 * chroma, baseSig = CX_SIG + (chroma ? 27 : 0);
    const int lastScanSet = scanPosLast >> 4;
    unsigned c1 = 1, goRice = 0;
    int scanPosSig = scanPosLast;
    for (int subSet = lastScanSet; subSet >= 0; subSet--) {
      int numNonZero = 0;
      const int subPos = subSet << 4;
      goRice = 0;
      unsigned coeffSigns = 0;
      int lastNZ = -1, firstNZ = 16;
      if (scanPosSig == scanPosLast) {
        const int c = coef[posLast];
        sh.absCoeff[0][lane] = (uint16_t)(c < 0 ? -c : c); coeffSigns = (c < 0); numNonZero = 1;
        lastNZ = scanPosSig; firstNZ = scanPosSig; scanPosSig--;
      }
      const int cgBlkPos = scanCG[subSet], cgPosY = cgBlkPos / numBlkSide, cgPosX = cgBlkPos - cgPosY * numBlkSide;
      unsigned r = 0, l = 0;
      if (cgPosX < numBlkSide - 1) r = (unsigned)((cgFlag >> (cgPosY * numBlkSide + cgPosX + 1)) & 1ull);
      if (cgPosY < numBlkSide - 1) l = (unsigned)((cgFlag >> ((cgPosY + 1) * numBlkSide + cgPosX)) & 1ull);
      if (subSet == lastScanSet || subSet == 0) cgFlag |= 1ull << cgBlkPos;
      else CBIN(baseCG + ((r || l) ? 1 : 0), (int)((cgFlag >> cgBlkPos) & 1ull));
      if ((cgFlag >> cgBlkPos) & 1ull) {
        const int patternSigCtx = (width == 4) ? -1 : (int)(r + (l << 1));
        for (; scanPosSig >= subPos; scanPosSig--) {
          const int blkPos = scan[scanPosSig], posY = blkPos >> log2, posX = blkPos - (posY << log2);
          const int c = coef[blkPos];
          const int sig = (c != 0);
          if (scanPosSig > subPos || subSet == 0 || numNonZero) {
            int ctxSig;                                            // getSigCtxInc, TComTrQuant.cpp:2038-2092
            if (posX + posY == 0) ctxSig = 0;
            else if (log2 == 2) ctxSig = hop_ctx_ind_map(4 * posY + posX);
            else {
              const int offset = log2 == 3 ? (scan_idx == 0 ? 9 : 15) : (!chroma ? 21 : 12);
              const int xs = posX & 3, ys = posY & 3;
              int cnt;
              if (patternSigCtx == 0) cnt = xs + ys <= 2 ? (xs + ys == 0 ? 2 : 1) : 0;
              else if (patternSigCtx == 1) cnt = ys <= 1 ? (ys == 0 ? 2 : 1) : 0;
              else if (patternSigCtx == 2) cnt = xs <= 1 ? (xs == 0 ? 2 : 1) : 0;
              else cnt = 2;
              ctxSig = ((!chroma && ((posX >> 2) + (posY >> 2)) > 0) ? 3 : 0) + offset + cnt;
            }
            CBIN(baseSig + ctxSig, sig);
          }
          if (sig) {
            const int a = c < 0 ? -c : c;
            sh.absCoeff[numNonZero][lane] = (uint16_t)a;                 // |TCoeff| <= 32768
            coeffSigns = 2 * coeffSigns + (c < 0);
            numNonZero++;
            if (lastNZ == -1) lastNZ = scanPosSig;
            firstNZ = scanPosSig;
          }
        }
      } else {
        scanPosSig = subPos - 1;
      }
      if (numNonZero > 0) {
        const int signHidden = (lastNZ - firstNZ >= 4);
        unsigned ctxSet = (subSet > 0 && !chroma) ? 2 : 0;
        if (c1 == 0) ctxSet++;
        c1 = 1;
        const int baseOne = CX_ONE + (chroma ? 16 : 0) + 4 * ctxSet;
        const int numC1 = numNonZero < 8 ? numNonZero : 8;
        int firstC2 = -1;
        for (int idx = 0; idx < numC1; idx++) {
          const int sym = sh.absCoeff[idx][lane] > 1;
          CBIN(baseOne + c1, sym);
          if (sym) { c1 = 0; if (firstC2 == -1) firstC2 = idx; }
          else if ((c1 < 3) && (c1 > 0)) c1++;
        }
        if (c1 == 0 && firstC2 != -1) CBIN(CX_ABS + (chroma ? 4 : 0) + ctxSet, sh.absCoeff[firstC2][lane] > 2);
        if (sign_hide && signHidden) frac += 32768ull * (unsigned long long)(numNonZero - 1);
        else frac += 32768ull * (unsigned long long)numNonZero;
        int firstCoeff2 = 1;
        if (c1 == 0 || numNonZero > 8) {
          for (int idx = 0; idx < numNonZero; idx++) {
            const int baseLevel = (idx < 8) ? (2 + firstCoeff2) : 1;
            const int a = sh.absCoeff[idx][lane];
            if (a >= baseLevel) {                                // xWriteCoefRemainExGolomb: only the number of bypass bins counts
              int codeNumber = a - baseLevel; unsigned length;
              if (codeNumber < (3 << goRice)) { length = (unsigned)codeNumber >> goRice; frac += 32768ull * (unsigned long long)(length + 1 + goRice); }
              else {
                length = goRice; codeNumber -= (3 << goRice);
                while (codeNumber >= (1 << length)) codeNumber -= (1 << (length++));
                frac += 32768ull * (unsigned long long)(3 + length + 1 - goRice + length);
              }
              if (a > 3 * (1 << goRice)) goRice = goRice + 1 < 4 ? goRice + 1 : 4;
            }
            if (a >= 2) firstCoeff2 = 0;
          }
        }
      }
    }
  }
  return frac;
}

__global__ __launch_bounds__(64) void k_coeff_bits(const hop_coeff_bits_job* __restrict__ jobs, int n, const hop_cabac_ctx* __restrict__ ctx_in,
                                                   const uint16_t* __restrict__ scans, const int32_t* __restrict__ coef_all,
                                                   unsigned long long* __restrict__ bits_out, hop_cabac_ctx* __restrict__ ctx_out) {
  __shared__ CabacLds sh;
  const int lane = threadIdx.x, j = blockIdx.x * 64 + lane;
  const bool inb = j < n;
  const hop_coeff_bits_job jb = jobs[inb ? j : 0];
  const bool live = inb && jb.log2_size >= 2;                         // < 2: an empty slot of a job table (k_rqt.inl)
  {
    const uint8_t* src = ctx_in[jb.ctx_index].state;
    for (int i = 0; i < 152; i++) sh.st[i][lane] = src[i];
  }
  const unsigned long long frac = live ? cb_code_tu(sh, lane, coef_all + jb.coeff_offset, jb.log2_size, jb.comp != 0, jb.scan_idx, jb.sign_hide, jb.use_ts, jb.ts_flag,
                                                   jb.cbf_ctx_plus1, scans) : 0ull;
  if (live) {
    bits_out[j] = frac;
    if (ctx_out) {
      uint8_t* dst = ctx_out[j].state;
      for (int i = 0; i < 150; i++) dst[i] = sh.st[i][lane];
      const unsigned left = ((unsigned)sh.st[150][lane] | ((unsigned)sh.st[151][lane] << 8)) + (unsigned)(frac & 32767ull);   // what resetBits will keep
      dst[150] = (uint8_t)(left & 0xFF); dst[151] = (uint8_t)((left >> 8) & 0x7F);
    }
  }
}

const int32_t* hop_entropy_bits_host(void) { return h_entropy_bits; }

int hop_launch_coeff_bits(hop_ctx* c, int n, const hop_coeff_bits_job* d_jobs, const hop_cabac_ctx* d_ctx, const int32_t* d_coef,
                          unsigned long long* d_bits, hop_cabac_ctx* d_ctx_out) {
  const int pr = hop_prof_begin(c, HOP_K_CABAC, (uint64_t)n);
  hipLaunchKernelGGL(k_coeff_bits, dim3((n + 63) / 64), dim3(64), 0, c->stream, d_jobs, n, d_ctx, c->rdoq_scans, d_coef, d_bits, d_ctx_out);
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "coeff_bits launch: %s", hipGetErrorString(e));
  return HOP_OK;
}

// ---- the mode-decision half of the intra rough search (rest of row a7): TEncSearch::estIntraPredQT :2440-2493 ----
// per block: for the 35 modes bits of the luma direction from the CI_CURR_BEST state (xModeBitsIntra :7734 = codeIntraDirLumaAng TEncSbac.cpp:770-831),
// cost = SATD + bits * sqrt(lambda) in double (:2461), the sorted candidate list (xUpdateCandList :7747-7767), the MPMs appended if missing (:2466-2488).
// ONE_LANE: called on one lane of a workgroup that holds the packed bin table in LDS (the candidate walks); otherwise a lane per block, the __constant__ table.
template <bool ONE_LANE>
__device__ static inline void intra_modes_body(const int i, const hop_intra_modes_job* jobs, const uint32_t* satd, hop_intra_modes_result* res) {
  const hop_intra_modes_job jb = jobs[i];
  const unsigned st = (unsigned)jb.ctx_state & 127u;                   // prev_intra_luma_pred_flag: its two bins' bits, once
  const unsigned long long bits_rem = ONE_LANE ? HOP_BIN_BITS(s_bin_table[(st << 1) | 0]) : (unsigned)c_entropy_bits[st ^ 0];
  const unsigned long long bits_mpm = ONE_LANE ? HOP_BIN_BITS(s_bin_table[(st << 1) | 1]) : (unsigned)c_entropy_bits[st ^ 1];
  const uint32_t* sd = satd + (size_t)i * 35;
  uint32_t modes[11]; double costs[8];
  const int nf = jb.num_full_rd;
  for (int q = 0; q < 11; q++) modes[q] = 0;
  for (int q = 0; q < 8; q++) costs[q] = 1.7e+308;
  const unsigned left = (unsigned)jb.frac_left & 32767u;
  for (int mode = 0; mode < 35; mode++) {
    int idx = -1;
    for (int q = 0; q < jb.pred_num; q++) if (mode == jb.preds[q]) idx = q;
    const unsigned long long frac = left + (idx != -1 ? bits_mpm : bits_rem) + 32768ull * (unsigned long long)(idx == -1 ? 5 : (idx ? 2 : 1));
    const double cost = (double)sd[mode] + (double)(uint32_t)(frac >> 15) * jb.sqrt_lambda;
    int shift = 0;
    while (shift < nf && cost < costs[nf - 1 - shift]) shift++;
    if (shift) {
      for (int q = 1; q < shift; q++) { modes[nf - q] = modes[nf - 1 - q]; costs[nf - q] = costs[nf - 1 - q]; }
      modes[nf - shift] = (uint32_t)mode; costs[nf - shift] = cost;
    }
  }
  int cnt = nf;
  for (int j = 0; j < jb.mpm_cand; j++) {
    bool inc = false;
    for (int q = 0; q < cnt; q++) inc |= (jb.preds[j] == (int)modes[q]);
    if (!inc) modes[cnt++] = (uint32_t)jb.preds[j];
  }
  hop_intra_modes_result r;
  r.n = (uint32_t)cnt;
  for (int q = 0; q < 11; q++) r.modes[q] = modes[q];
  for (int q = 0; q < 8; q++) r.costs[q] = costs[q];
  res[i] = r;
}
__global__ void k_intra_modes(const hop_intra_modes_job* __restrict__ jobs, int n, const uint32_t* __restrict__ satd, hop_intra_modes_result* __restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) intra_modes_body<false>(i, jobs, satd, res);
}
int hop_launch_intra_modes(hop_ctx* c, int n, const hop_intra_modes_job* d_jobs, const uint32_t* d_satd, hop_intra_modes_result* d_res) {
  const int pr = hop_prof_begin(c, HOP_K_INTRA, 0);
  hipLaunchKernelGGL(k_intra_modes, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_jobs, n, d_satd, d_res);
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "intra_modes launch: %s", hipGetErrorString(e));
  return HOP_OK;
}

#include "k_intra_dev.inl"
#include "k_walk_stamps.inl"
#include "k_leaf_fused.inl"
#include "k_rqt.inl"
#include "k_walk.inl"

// ---- the stage stamps' table (k_walk_stamps.inl) read back: hop_walk_stamps_* of include/hophip.h ----
const char* hop_walk_stamps_stage_name(int stage) {
  static const char* const names[HOP_WS_COUNT] = { "LEAF_FORWARD", "LEAF_ESTBITS", "LEAF_RDOQ", "LEAF_BITS", "LEAF_WAIT", "LEAF_INVERSE", "LEAF_DECIDE", "NODE_BEGIN", "NODE_SINGLE",
                                                   "NODE_CLOSE", "PREDICT", "COPY", "TAIL", "CU_BITS", "OTHER" };
  return stage >= 0 && stage < HOP_WS_COUNT ? names[stage] : nullptr;
}
#ifndef HOP_WALK_STAMPS
static int ws_refuse(hop_ctx* c, const char* what) {
  return hop_set_err(c, HOP_ERR_STATE, "%s: this library holds no stamps; load libhophip_stamps.so (the diagnostic build of csrc/k_cabac.hip; HOP_LIB for hophip.py)", what);
}
int hop_walk_stamps_read(hop_ctx* c, int, int, int, uint64_t*, uint64_t*, hop_walk_stamps_total*) { return ws_refuse(c, "hop_walk_stamps_read"); }
int hop_walk_stamps_reset(hop_ctx* c) { return ws_refuse(c, "hop_walk_stamps_reset"); }
int hop_walk_stamps_probe(hop_ctx* c, uint64_t*) { return ws_refuse(c, "hop_walk_stamps_probe"); }
#else
// the context's device, and everything queued on its streams done (the classes of a *_device_classes call run on the extra lanes too)
static int ws_quiesce(hop_ctx* c, const char* what) {
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  for (int l = 0; l + 1 < c->lanes && l < HOP_MAX_LANES - 1 && e == hipSuccess; l++) if (c->xlane[l].stream) e = hipStreamSynchronize(c->xlane[l].stream);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  return HOP_OK;
}
int hop_walk_stamps_read(hop_ctx* c, int kernel, int log2_cu, int nxn, uint64_t* cycles, uint64_t* visits, hop_walk_stamps_total* total) {
  if (!c) return HOP_ERR_ARG;
  if (kernel < 0 || kernel >= HOP_WSK_COUNT || log2_cu < 3 || log2_cu > 6 || nxn < 0 || nxn > 1)
    return hop_set_err(c, HOP_ERR_ARG, "hop_walk_stamps_read: kernel %d (0..%d), log2_cu %d (3..6), nxn %d (0 / 1)", kernel, HOP_WSK_COUNT - 1, log2_cu, nxn);
  int r = ws_quiesce(c, "hop_walk_stamps_read"); if (r) return r;
  unsigned long long row[WS_ROW];
  const size_t at = ((((size_t)kernel * 4 + (log2_cu - 3)) * 2) + nxn) * sizeof(row);
  hipError_t e = hipMemcpyFromSymbol(row, HIP_SYMBOL(g_ws_table), sizeof(row), at, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "hop_walk_stamps_read: %s", hipGetErrorString(e));
  for (int s = 0; s < HOP_WS_COUNT; s++) { if (cycles) cycles[s] = row[s]; if (visits) visits[s] = row[HOP_WS_COUNT + s]; }
  if (total) { total->workgroups = row[2 * HOP_WS_COUNT]; total->cycles = row[2 * HOP_WS_COUNT + 1]; total->realtime_ticks = row[2 * HOP_WS_COUNT + 2]; total->max_realtime_ticks = row[2 * HOP_WS_COUNT + 3]; }
  return HOP_OK;
}
int hop_walk_stamps_reset(hop_ctx* c) {
  if (!c) return HOP_ERR_ARG;
  int r = ws_quiesce(c, "hop_walk_stamps_reset"); if (r) return r;
  void* p = nullptr;
  hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_ws_table));
  if (e == hipSuccess) e = hipMemset(p, 0, sizeof(unsigned long long) * HOP_WSK_COUNT * 4 * 2 * WS_ROW);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "hop_walk_stamps_reset: %s", hipGetErrorString(e));
  return HOP_OK;
}
int hop_walk_stamps_probe(hop_ctx* c, uint64_t* out) {
  if (!c || !out) return hop_set_err(c, HOP_ERR_ARG, "hop_walk_stamps_probe: NULL argument");
  int r = ws_quiesce(c, "hop_walk_stamps_probe"); if (r) return r;
  hipLaunchKernelGGL(k_ws_probe, dim3(1), dim3(256), 0, c->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  unsigned long long v[4];
  if (e == hipSuccess) e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_ws_probe), sizeof(v), 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "hop_walk_stamps_probe: %s", hipGetErrorString(e));
  for (int q = 0; q < 4; q++) out[q] = v[q];
  return HOP_OK;
}
#endif
