// k_leaf_fused.inl -- the transform-unit leaf step (row a8b: residual, xT, estBit, RDOQ, counted bits, inverse path, cbf-zero decision; the stages of hop_launch_tu_rd)
// as ONE kernel, one workgroup per TU.  Included by k_cabac.hip.
// The staged pipeline of k_tq.hip / k_rdoq.hip is 13 launches per batch and lays its serial stages (RDOQ, bit counting) out one LANE per TU: right for the thousands of
// TUs of a frozen-reference search, wrong for the RD spine, whose batches hold one TU per CTU in flight and which walks a chain of thousands of such batches per CTU -- there
// the launches ARE the time.  Here a workgroup takes its TU through all stages: the transforms on all 256 threads (or one wave for 4x4 / 8x8), the serial stages on thread 0
// in between.  The arithmetic is the staged kernels' own (the shared bodies of k_turd_dev.inl, k_rdoq_dev.inl, cb_code_tu), so the results are identical by construction;
// tests/test_gpu_tq_intra.py runs both.
#include "k_turd_dev.inl"
#include "k_rdoq_dev.inl"
#include "k_quant_flat_dev.inl"

#define LEAF_WORK_PER_TU ((size_t)1024 * RQ_WORK_PER_COEF)           // the RDOQ work area of a 32x32 TU at ws = 1

struct LeafShared {
  union { TurdFwdShared big; TurdSmallShared small; } t;
  CabacLds1 cab;                                                      // the TU's context states
  uint16_t scan[1024]; uint16_t scanCG[64]; double cgSig[64];
  // everything the serial walk touches (a lane's dependent loads from HBM were most of its time): coefficients, levels, bit-estimate table, context states, the
  // entropy table, and the RDOQ work area of TUs up to 16x16 (a 32x32 TU's 40 KB stay in HBM)
  int32_t src[1024], lev[1024], ebits[128]; hop_estbits eb; uint8_t ctx[152]; double work[256 * RQ_WORK_PER_COEF / 8];
  // the job records of the serial stages (also written to rq[j] / cb[j]) and what RDOQ's phases hand on
  hop_rdoq_job rj; hop_coeff_bits_job bj; union { RqPhase ph; QfPhase qf; }; uint16_t cgMask[64];      // (qf: a unit that does not use RDOQ, leaf_flat_*)
  // what RDOQ's preparation hands to the serial lane, in LDS for every size: |coefficient| * Q, the cost of coding nothing, the significance contexts (16 KB)
  int32_t plvl[1024]; double pcost[1024]; int32_t pctx[1024];
};

// The serial stages of one transform unit on the calling lane, as FUNCTIONS OF THEIR OWN: leaf_serial, the recurrence of RDOQ (rdoq_serial, k_rdoq_dev.inl), and leaf_bits,
// the counted bits.  Inlined into a candidate walk they shared the walk's register budget with everything the walk keeps live around them, and the compiler spilled into the
// per-coefficient loops (a reload is a vector-memory load on the dependent path).  As functions the loops get a register allocation of their own and the caller's live state is
// saved once around the call.  No barrier inside: the calls stand under `if (lane == 0)`.  L is the caller's LeafShared / LeafSmallShared in LDS (hopd_lds: the loops address
// it with ds_* instructions, not flat_*).  MAXLOG2 = 5: a 32x32 unit's RDOQ work area is `wd`, its slot of the work buffer in HBM; smaller units use L.work.  The counted bits
// read the workgroup's bin table (cab_bin_fill at the kernel's entry).
// Between the two stand RDOQ's finishing phases on all lanes (signs, sign-bit hiding, the scatter into L.lev): the counted bits read the finished levels.
struct LeafSmallShared;
__device__ static __forceinline__ RqPrep leaf_prep_arrays(LeafShared& L) { RqPrep pp; pp.lvlD = L.plvl; pp.cost0 = L.pcost; pp.ctx = L.pctx; return pp; }
__device__ static __forceinline__ RqPrep leaf_prep_arrays(LeafSmallShared& L);                    // (a wave's unit: inside its work area)
template <class SH, int MAXLOG2>
__device__ __noinline__ static void leaf_serial(SH* Lg, const int LOG2, double* wd) {
  SH& L = *hopd_lds(Lg);
  if (LOG2 == 2) rdoq_serial<2>(L.rj, &L.eb, L.scan, L.scanCG, L.cgSig, L.cgMask, &L.ph, L.work, leaf_prep_arrays(L));
  else if (MAXLOG2 == 3 || LOG2 == 3) rdoq_serial<3>(L.rj, &L.eb, L.scan, L.scanCG, L.cgSig, L.cgMask, &L.ph, L.work, leaf_prep_arrays(L));
  else if (LOG2 == 4) rdoq_serial<4>(L.rj, &L.eb, L.scan, L.scanCG, L.cgSig, L.cgMask, &L.ph, L.work, leaf_prep_arrays(L));
  else rdoq_serial<5>(L.rj, &L.eb, L.scan, L.scanCG, L.cgSig, L.cgMask, &L.ph, wd, leaf_prep_arrays(L));
}
template <class SH>
__device__ __noinline__ static void leaf_bits(SH* Lg, unsigned long long* fr_j) {
  SH& L = *hopd_lds(Lg);
  const hop_coeff_bits_job bj = L.bj;
  *fr_j = cb_code_tu_at(L.cab, 0, L.lev, bj.log2_size, bj.comp != 0, bj.scan_idx, bj.sign_hide, bj.use_ts, bj.ts_flag, bj.cbf_ctx_plus1, L.scan, L.scanCG);
}

// The serial stages' share of all lanes, in pieces with the serial lane's two calls between them.  Every lane that serves the unit calls each piece (`lane` of `nlanes`);
// the pieces hold no barrier: LEAF_SYNC() below, the workgroup's barrier, stands between them in the bodies, where every thread of the workgroup reaches it.
//   leaf_records: the job records, on one lane beside the loads: rq[j] / cb[j] as turd_setup_body writes them, and the copies in LDS that every later piece and the serial
//                 lane read -- no read-back from HBM
//   leaf_prepare: the bit-estimate table (a word per lane and step), RDOQ's per-position preparation
//   leaf_groups:  RDOQ's per-group preparation and the last significant position
//   leaf_finish1 / leaf_finish2 / leaf_finish3: signs and sum | sign-bit hiding | the scatter into L.lev and abs_sum
// Like leaf_serial they are functions of their own (inlined at every leaf of a walk they cost the walk kernels a hundred more spilled registers); the table of DESIGN.md
// section 4 has both.  wd is L.work or a 32x32 unit's slot in HBM: generic, flat_* on lanes that work side by side.
#define LEAF_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)
template <class SH>
__device__ static __forceinline__ void leaf_records(SH& L, const hop_tu_rd_job& jb, const int j, const int64_t off, hop_rdoq_job* rq, hop_coeff_bits_job* cb) {
  hop_rdoq_job rj; hop_coeff_bits_job bj;
  turd_records_make(jb, j, off, rj, bj);
  L.rj = rj; L.bj = bj; rq[j] = rj; cb[j] = bj;
  L.qf.absSum = 0; L.qf.topSubset = -1;                               // (what leaf_flat_levels adds into.  Unconditional on purpose: under `if (flat)` k_inter_walk and k_iw_cand gain scratch and spills; a unit that uses RDOQ re-initialises these words, its RqPhase, in rdoq_prep_pos behind the barrier)
}
template <class SH>
__device__ __noinline__ static void leaf_prepare(SH* Lg, const int lane, const int nlanes, double* wd) {
  SH& L = *hopd_lds(Lg);
  WS(HOP_WS_LEAF_ESTBITS);
  turd_estbits_fill(lane, nlanes, L.rj.log2_size, L.rj.comp, L.ctx, L.ebits, &L.eb);
  WS(HOP_WS_LEAF_RDOQ);
  rdoq_prep_pos(L.rj, L.scan, L.src, leaf_prep_arrays(L), &L.ph, lane, nlanes);
}
template <class SH>
__device__ __noinline__ static void leaf_groups(SH* Lg, const int lane, const int nlanes, double* wd) { SH& L = *hopd_lds(Lg); rdoq_prep_groups(L.rj, L.cgMask, leaf_prep_arrays(L), &L.ph, lane, nlanes); }
template <class SH>
__device__ __noinline__ static void leaf_finish1(SH* Lg, const int lane, const int nlanes, double* wd) { SH& L = *hopd_lds(Lg); rdoq_finish_levels(L.rj, L.scan, L.src, wd, &L.ph, lane, nlanes); }
template <class SH>
__device__ __noinline__ static void leaf_finish2(SH* Lg, const int lane, const int nlanes, double* wd) { SH& L = *hopd_lds(Lg); rdoq_finish_sbh(L.rj, L.scan, L.src, wd, &L.ph, lane, nlanes); }
template <class SH>
__device__ __noinline__ static void leaf_finish3(SH* Lg, const int lane, const int nlanes, uint32_t* as_j, double* wd) {
  SH& L = *hopd_lds(Lg);
  rdoq_finish_scatter(L.rj, L.scan, L.lev, as_j, wd, &L.ph, lane, nlanes);
}

// A unit that does not use RDOQ (hop_ctx_set_quant_mode; the rule of xQuant, TComTrQuant.cpp:1012: by its transform-skip flag): the plain quantiser and the reference's
// sign-bit hiding of that branch (k_quant_flat_dev.inl) on all lanes, in the place of leaf_prepare ... leaf_finish3 and with no call on the serial lane.  No bit-estimate
// table: only RDOQ reads one.  The remainders deltaU go where RDOQ's preparation would have gone (plvl / the work area).  Uniform over the lanes that serve the unit.
__device__ static __forceinline__ bool leaf_is_flat(const hop_pics& pic, const hop_tu_rd_job& jb) { return (pic.quant_mode & ((jb.flags & HOP_TU_RD_TS) ? HOP_QM_FLAT_TS : HOP_QM_FLAT)) != 0; }
__device__ static __forceinline__ int32_t* leaf_flat_du(LeafShared& L) { return L.plvl; }
__device__ static __forceinline__ int32_t* leaf_flat_du(LeafSmallShared& L);
template <class SH>
__device__ static __forceinline__ QfUnit leaf_flat_unit(SH& L, const int i_slice) {
  QfUnit u; u.log2_size = L.rj.log2_size; u.qp_scaled = L.rj.qp_scaled; u.bit_depth = L.rj.bit_depth; u.i_slice = i_slice; u.sign_hide = L.rj.sign_hide;
  return u;
}
template <class SH>
__device__ __noinline__ static void leaf_flat_levels(SH* Lg, const int lane, const int nlanes, const int i_slice) {
  SH& L = *hopd_lds(Lg);
  WS(HOP_WS_LEAF_RDOQ);
  quant_flat_levels(leaf_flat_unit(L, i_slice), L.scan, L.src, L.lev, leaf_flat_du(L), &L.qf, lane, nlanes);
}
template <class SH>
__device__ __noinline__ static void leaf_flat_sbh(SH* Lg, const int lane, const int nlanes, const int i_slice, uint32_t* as_j) {
  SH& L = *hopd_lds(Lg);
  quant_flat_sbh(leaf_flat_unit(L, i_slice), L.scan, L.src, L.lev, leaf_flat_du(L), as_j, &L.qf, lane, nlanes);
}

// one TU through all stages on the 256 threads of the calling workgroup (every thread calls; barriers inside)
__device__ static void turd_fused_body(LeafShared& L_, const int j, const hop_tu_rd_job* jobs, int n, hop_pics pic, const hop_cabac_ctx* ctx_in, const int64_t* coef_off,
                                       const int32_t* entropy_bits, const uint16_t* scans, int32_t* coef, int32_t* levels, uint32_t* zs, uint32_t* ns, uint32_t* as,
                                       unsigned long long* fr, hop_rdoq_job* rq, hop_coeff_bits_job* cb, char* work, hop_tu_rd_result* res, int16_t* rec_y, int16_t* rec_cb, int16_t* rec_cr) {
  LeafShared& L = *hopd_lds(&L_);                                     // (where the compiler makes this body a function of its own, &L_ arrives as a generic pointer)
  const int tid = threadIdx.x;
  const hop_tu_rd_job jb = jobs[j];
  if (jb.log2_size < 2 || jb.log2_size > 5) return;                   // an empty slot of a job table (k_rqt.inl); uniform over the workgroup
  const bool small = jb.log2_size <= 3;
  const bool flat = leaf_is_flat(pic, jb);                            // (mode and job: uniform over the workgroup)
  const int i_slice = (pic.quant_mode & HOP_QM_I_SLICE) != 0;
  const int LOG2 = jb.log2_size, N2 = 1 << (2 * LOG2), CGN = N2 >> 4;
  WS(HOP_WS_LEAF_FORWARD);
  // residual, forward transform (or the transform-skip scaling), distortion of the zero block
  if (small) { if (tid < 64) turd_forward_small_body(L.t.small, 0, tid, j, jobs, n, pic, coef_off, coef, zs); }
  else turd_forward_body(L.t.big, j, jobs, pic, coef_off, coef, zs);
  { const uint16_t* s0 = rq_scan(scans, jb.scan_idx, LOG2); const uint16_t* s1 = rq_scan_cg(scans, jb.scan_idx, LOG2);
    for (int i = tid; i < N2; i += 256) L.scan[i] = s0[i];
    for (int i = tid; i < CGN; i += 256) L.scanCG[i] = s1[i]; }
  __threadfence_block();
  __syncthreads();
  const int64_t off = coef_off[j];
  for (int i = tid; i < N2; i += 256) L.src[i] = coef[off + i];
  { const uint8_t* st = ctx_in[jb.ctx_index].state; for (int i = tid; i < 152; i += 256) { const uint8_t v = st[i]; L.ctx[i] = v; L.cab.st[i][0] = v; } }
  for (int i = tid; i < 128; i += 256) L.ebits[i] = entropy_bits[i];
  if (tid == 255) leaf_records(L, jb, j, off, rq, cb);
  __syncthreads();
  // the serial stages: what depends on the position alone on all threads, the recurrences on thread 0
  double* const wd = LOG2 == 5 ? (double*)(work + (size_t)j * LEAF_WORK_PER_TU) : L.work;
  // (every barrier stands where all threads reach it, whichever quantiser the unit takes)
  if (flat) leaf_flat_levels(&L, tid, 256, i_slice); else leaf_prepare(&L, tid, 256, wd);
  LEAF_SYNC();
  if (flat) leaf_flat_sbh(&L, tid, 256, i_slice, as + j); else leaf_groups(&L, tid, 256, wd);
  LEAF_SYNC();
  if (!flat && tid == 0) leaf_serial<LeafShared, 5>(&L, LOG2, wd);
  LEAF_SYNC();                                                        // (RDOQ's three parts are one visit of LEAF_RDOQ on thread 0's timeline)
  if (!flat) leaf_finish1(&L, tid, 256, wd);
  LEAF_SYNC();
  if (!flat) leaf_finish2(&L, tid, 256, wd);
  LEAF_SYNC();
  if (!flat) leaf_finish3(&L, tid, 256, as + j, wd);
  LEAF_SYNC();
  WS(HOP_WS_LEAF_BITS);
  for (int i = tid; i < N2; i += 256) levels[off + i] = L.lev[i];     // (beside thread 0's count: both only read L.lev)
  if (tid == 0) leaf_bits<LeafShared>(&L, fr + j);
  WS(HOP_WS_LEAF_WAIT);
  __threadfence_block();
  __syncthreads();
  WS(HOP_WS_LEAF_INVERSE);
  // dequantisation, inverse transform, reconstruction (intra) and the distortion of the coded block
  if (small) { if (tid < 64) turd_inverse_small_body(L.t.small, 0, tid, j, jobs, n, pic, coef_off, levels, as, ns, rec_y, rec_cb, rec_cr); }
  else turd_inverse_body(L.t.big, j, jobs, pic, coef_off, levels, as, ns, rec_y, rec_cb, rec_cr);
  __threadfence_block();
  __syncthreads();
  WS(HOP_WS_LEAF_DECIDE);
  if (tid == 0) turd_decide_body(j, jobs, n, ctx_in, coef_off, entropy_bits, as, fr, zs, ns, levels, res);
}
__global__ __launch_bounds__(256) void k_turd_fused(const hop_tu_rd_job* __restrict__ jobs, int n, hop_pics pic, const hop_cabac_ctx* __restrict__ ctx_in,
                                                    const int64_t* __restrict__ coef_off, const int32_t* __restrict__ entropy_bits, const uint16_t* __restrict__ scans,
                                                    int32_t* __restrict__ coef, int32_t* __restrict__ levels, uint32_t* __restrict__ zs, uint32_t* __restrict__ ns,
                                                    uint32_t* __restrict__ as, unsigned long long* __restrict__ fr, hop_estbits* __restrict__ tables,
                                                    hop_rdoq_job* __restrict__ rq, hop_coeff_bits_job* __restrict__ cb, char* __restrict__ work,
                                                    hop_tu_rd_result* __restrict__ res, int16_t* __restrict__ rec_y, int16_t* __restrict__ rec_cb, int16_t* __restrict__ rec_cr) {
  __shared__ LeafShared L;
  cab_bin_fill();                                                     // the counted bits' bin table (all threads; the barrier is inside)
  turd_fused_body(L, blockIdx.x, jobs, n, pic, ctx_in, coef_off, entropy_bits, scans, coef, levels, zs, ns, as, fr, rq, cb, work, res, rec_y, rec_cb, rec_cr);
}

// The same for batches whose TUs are all 4x4 or 8x8 (size_hint 1: most of the quadtree steps of 8x8 CUs, every chroma step of CUs up to 16x16): ONE wave per TU and
// 1.6 KB of LDS, so that a compute unit holds 32 TUs instead of 7 -- in the large batches of many CTUs in flight the leaf step is bound by how many serial walks the
// GPU holds at once.
struct LeafSmallShared { TurdSmallShared t; CabacLds1 cab; uint16_t scan[64]; uint16_t scanCG[4]; double cgSig[4];
                         double work[64 * RQ_WORK_PER_COEF / 8]; hop_estbits eb; int32_t src[64], lev[64], ebits[128]; uint8_t ctx[152];   // everything the serial walk touches
                         hop_rdoq_job rj; hop_coeff_bits_job bj; union { RqPhase ph; QfPhase qf; }; uint16_t cgMask[4]; };
__device__ static __forceinline__ RqPrep leaf_prep_arrays(LeafSmallShared& L) { return rq_prep_in_work(L.work, 1 << (2 * L.rj.log2_size)); }
__device__ static __forceinline__ int32_t* leaf_flat_du(LeafSmallShared& L) { return (int32_t*)L.work; }

// The same body for the candidate walks (k_walk.inl): up to four small transform units of one tree node side by side, one per WAVE of the 256-thread workgroup, each with
// its own LeafSmallShared; k_turd_fused_small is this body on a workgroup of one wave.  Every wave calls (the barriers are the workgroup's); a wave without a unit passes
// j < 0 and only keeps step.  EVERY barrier stands outside `if (live)`: all threads of the workgroup reach each of them, whatever their wave's unit (a barrier inside a body
// reached through wave-divergent control flow is undefined behaviour; the first form of this body aborted on the device with a memory aperture violation).
__device__ static __forceinline__ void turd_fused_small_wave_body(LeafSmallShared& L, const int lane, const int j, const hop_tu_rd_job* jobs, int n, hop_pics pic, const hop_cabac_ctx* ctx_in,
                                                  const int64_t* coef_off, const int32_t* entropy_bits, const uint16_t* scans, int32_t* coef, int32_t* levels, uint32_t* zs, uint32_t* ns,
                                                  uint32_t* as, unsigned long long* fr, hop_rdoq_job* rq, hop_coeff_bits_job* cb, hop_tu_rd_result* res, int16_t* rec_y, int16_t* rec_cb,
                                                  int16_t* rec_cr) {
  hop_tu_rd_job jb; jb.log2_size = 0; jb.scan_idx = 0; jb.ctx_index = 0;
  if (j >= 0) jb = jobs[j];
  const bool live = j >= 0 && jb.log2_size >= 2 && jb.log2_size <= 3;      // (uniform over the wave)
  const int LOG2 = live ? jb.log2_size : 2, N2 = 1 << (2 * LOG2), CGN = N2 >> 4;
  const bool flat = live && leaf_is_flat(pic, jb), rdoq = live && !flat;      // (uniform over the wave; the waves of a workgroup may differ: a unit beside its transform-skip twin)
  const int i_slice = (pic.quant_mode & HOP_QM_I_SLICE) != 0;
  int64_t off = 0;
  WS(HOP_WS_LEAF_FORWARD);
  if (live) {
    turd_forward_small_body(L.t, 0, lane, j, jobs, n, pic, coef_off, coef, zs);
    const uint16_t* s0 = rq_scan(scans, jb.scan_idx, LOG2); const uint16_t* s1 = rq_scan_cg(scans, jb.scan_idx, LOG2);
    if (lane < N2) L.scan[lane] = s0[lane];
    if (lane < CGN) L.scanCG[lane] = s1[lane];
  }
  __threadfence_block();
  __syncthreads();
  if (live) {
    off = coef_off[j];
    if (lane < N2) L.src[lane] = coef[off + lane];
    const uint8_t* st = ctx_in[jb.ctx_index].state; for (int i = lane; i < 152; i += 64) { const uint8_t v = st[i]; L.ctx[i] = v; L.cab.st[i][0] = v; }
    for (int i = lane; i < 128; i += 64) L.ebits[i] = entropy_bits[i];
    if (lane == 63) leaf_records(L, jb, j, off, rq, cb);
  }
  __syncthreads();
  // the serial stages: what depends on the position alone on the wave's 64 lanes, the recurrences on its lane 0
  if (flat) leaf_flat_levels(&L, lane, 64, i_slice); else if (rdoq) leaf_prepare(&L, lane, 64, L.work);
  LEAF_SYNC();
  if (flat) leaf_flat_sbh(&L, lane, 64, i_slice, as + j); else if (rdoq) leaf_groups(&L, lane, 64, L.work);
  LEAF_SYNC();
  if (rdoq && lane == 0) leaf_serial<LeafSmallShared, 3>(&L, LOG2, L.work);
  LEAF_SYNC();                                                          // (thread 0 waits here for the other waves' serial lanes: part of its one visit of LEAF_RDOQ)
  if (rdoq) leaf_finish1(&L, lane, 64, L.work);
  LEAF_SYNC();
  if (rdoq) leaf_finish2(&L, lane, 64, L.work);
  LEAF_SYNC();
  if (rdoq) leaf_finish3(&L, lane, 64, as + j, L.work);
  LEAF_SYNC();
  WS_IF(live, HOP_WS_LEAF_BITS);
  if (live && lane < N2) levels[off + lane] = L.lev[lane];              // (beside lane 0's count: both only read L.lev)
  if (live && lane == 0) leaf_bits<LeafSmallShared>(&L, fr + j);
  WS(HOP_WS_LEAF_WAIT);
  __threadfence_block();
  __syncthreads();
  WS(HOP_WS_LEAF_INVERSE);
  if (live) turd_inverse_small_body(L.t, 0, lane, j, jobs, n, pic, coef_off, levels, as, ns, rec_y, rec_cb, rec_cr);
  __threadfence_block();
  __syncthreads();
  WS_IF(live, HOP_WS_LEAF_DECIDE);
  if (live && lane == 0) turd_decide_body(j, jobs, n, ctx_in, coef_off, entropy_bits, as, fr, zs, ns, levels, res);
}

__global__ __launch_bounds__(64) void k_turd_fused_small(const hop_tu_rd_job* __restrict__ jobs, int n, hop_pics pic, const hop_cabac_ctx* __restrict__ ctx_in,
                                                         const int64_t* __restrict__ coef_off, const int32_t* __restrict__ entropy_bits, const uint16_t* __restrict__ scans,
                                                         int32_t* __restrict__ coef, int32_t* __restrict__ levels, uint32_t* __restrict__ zs, uint32_t* __restrict__ ns,
                                                         uint32_t* __restrict__ as, unsigned long long* __restrict__ fr, hop_estbits* __restrict__ tables,
                                                         hop_rdoq_job* __restrict__ rq, hop_coeff_bits_job* __restrict__ cb, char* __restrict__ work,
                                                         hop_tu_rd_result* __restrict__ res, int16_t* __restrict__ rec_y, int16_t* __restrict__ rec_cb, int16_t* __restrict__ rec_cr) {
  __shared__ LeafSmallShared L;
  cab_bin_fill();                                                     // (all threads; the barrier is inside)
  // the wave body on a workgroup of one wave; an empty slot (or a larger TU, which never comes here: size_hint 1) keeps step through its barriers and does nothing
  turd_fused_small_wave_body(L, threadIdx.x, blockIdx.x, jobs, n, pic, ctx_in, coef_off, entropy_bits, scans, coef, levels, zs, ns, as, fr, rq, cb, res, rec_y, rec_cb, rec_cr);
}

size_t hop_tu_rd_fused_scratch(int n, size_t n_coeff) {
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  return al(n_coeff * 4) + 4 * al((size_t)n * 4) + al((size_t)n * 8) + al((size_t)n * sizeof(hop_estbits)) + al((size_t)n * sizeof(hop_rdoq_job)) +
         al((size_t)n * sizeof(hop_coeff_bits_job)) + (size_t)n * LEAF_WORK_PER_TU + 256;
}

int hop_launch_tu_rd_fused(hop_ctx* c, int n, const hop_tu_rd_job* d_jobs, const hop_cabac_ctx* d_ctx, const int64_t* d_coef_off, size_t n_coeff,
                           int32_t* d_levels, hop_tu_rd_result* d_res, int all_small) {
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_coef = 0, o_zs = al(o_coef + n_coeff * 4), o_ns = al(o_zs + (size_t)n * 4), o_as = al(o_ns + (size_t)n * 4), o_fr = al(o_as + (size_t)n * 4);
  const size_t o_tab = al(o_fr + (size_t)n * 8), o_rq = al(o_tab + (size_t)n * sizeof(hop_estbits)), o_cb = al(o_rq + (size_t)n * sizeof(hop_rdoq_job));
  const size_t o_wk = al(o_cb + (size_t)n * sizeof(hop_coeff_bits_job));
  void* sc; int r = hop_scratch(c, o_wk + (size_t)n * LEAF_WORK_PER_TU + 256, &sc); if (r) return r;
  char* b = (char*)sc;
  const int pr = hop_prof_begin(c, HOP_K_TQ, (uint64_t)n);
  if (all_small)
    hipLaunchKernelGGL(k_turd_fused_small, dim3(n), dim3(64), 0, c->stream, d_jobs, n, hop_make_pics(c), d_ctx, d_coef_off, hop_entropy_bits_device(c), c->rdoq_scans,
                       (int32_t*)(b + o_coef), d_levels, (uint32_t*)(b + o_zs), (uint32_t*)(b + o_ns), (uint32_t*)(b + o_as), (unsigned long long*)(b + o_fr),
                       (hop_estbits*)(b + o_tab), (hop_rdoq_job*)(b + o_rq), (hop_coeff_bits_job*)(b + o_cb), b + o_wk, d_res, c->rec[0], c->rec[1], c->rec[2]);
  else
  hipLaunchKernelGGL(k_turd_fused, dim3(n), dim3(256), 0, c->stream, d_jobs, n, hop_make_pics(c), d_ctx, d_coef_off, hop_entropy_bits_device(c), c->rdoq_scans,
                     (int32_t*)(b + o_coef), d_levels, (uint32_t*)(b + o_zs), (uint32_t*)(b + o_ns), (uint32_t*)(b + o_as), (unsigned long long*)(b + o_fr),
                     (hop_estbits*)(b + o_tab), (hop_rdoq_job*)(b + o_rq), (hop_coeff_bits_job*)(b + o_cb), b + o_wk, d_res, c->rec[0], c->rec[1], c->rec[2]);
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "tu_rd (fused) launch: %s", hipGetErrorString(e));
  return HOP_OK;
}
