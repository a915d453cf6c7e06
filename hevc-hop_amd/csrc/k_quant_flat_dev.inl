// k_quant_flat_dev.inl -- the quantiser of a transform unit that does NOT use RDOQ (hop_ctx_set_quant_mode): the plain branch of TComTrQuant::xQuant
// (TLibCommon/TComTrQuant.cpp:1071-1116, flat scaling list) with TComTrQuant::signBitHidingHDQ (:868-990), for a unit that has lanes to itself (the leaf bodies of
// k_leaf_fused.inl, the staged k_quant_flat of k_tq.hip).  Plain C++ over include/hophip.h: host/hop_quant_flat_host.cpp compiles it with __device__ defined away
// (hop_quant_flat_tu_host) and tests/test_quant_mode_cpu.py compares it with the reference's own blocks.
// Nothing here is a recurrence.  Two functions of (lane, nlanes), a barrier of the lanes that serve the unit between them (the caller's: neither holds one):
//   quant_flat_levels: a scan position per lane and step -- the level (level = (|c| * Q + offset) >> qBits, offset = 171 or 85 in 1/512 of a step), the remainder deltaU
//                      in 1/256 of a step, the clip to 16 bit; the sum of the levels before the clip (uiAcSum) and the highest coefficient group of the scan that holds
//                      a level (an integer sum and a maximum over lanes: any order)
//   quant_flat_sbh:    a coefficient group per lane and step.  The reference walks the groups downwards and treats the first one that holds a level as the last group
//                      (lastCG == 1: its candidates end at its last level instead of position 15); a group without a level is never changed and a changed group's levels
//                      are its own, so that group is the highest one holding a level before any change: ph->topSubset.  Inside a group the reference's loop runs from the
//                      top position down and replaces the minimum on a strict `<`: among equal costs the highest scan position wins, as here.
// ph is initialised by the caller before the barrier that precedes quant_flat_levels ({ 0, -1 }).  lev and du are raster N x N like src.
struct QfPhase { uint32_t absSum; int topSubset; };
struct QfUnit { int log2_size, qp_scaled, bit_depth, i_slice, sign_hide; };
#if defined(QF_HOST)
#define QF_MAX_INTO(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)  // (emulated lanes run one after the other)
#define QF_ADD_INTO(p, v) (*(p) += (v))
#else
#define QF_MAX_INTO(p, v) atomicMax((p), (v))
#define QF_ADD_INTO(p, v) atomicAdd((p), (v))
#endif
__device__ static inline int qf_quant_scale(int rem) { return rem == 0 ? 26214 : rem == 1 ? 23302 : rem == 2 ? 20560 : rem == 3 ? 18396 : rem == 4 ? 16384 : 14564; }   // TComRom.cpp:164-167

__device__ static inline void quant_flat_levels(const QfUnit& u, const uint16_t* scan, const int32_t* src, int32_t* lev, int32_t* du, QfPhase* ph, const int lane, const int nlanes) {
  const int N2 = 1 << (2 * u.log2_size);
  const int per = u.qp_scaled / 6, rem = u.qp_scaled % 6;
  const int qBits = 14 + per + (15 - u.bit_depth - u.log2_size), q = qf_quant_scale(rem);
  const long long add = (long long)(u.i_slice ? 171 : 85) << (qBits - 9);
  uint32_t sum = 0; int top = -1;
  for (int sp = lane; sp < N2; sp += nlanes) {
    const int blkPos = scan[sp];
    const int c = src[blkPos];
    const long long t = (long long)(c < 0 ? -(long long)c : (long long)c) * q;
    const int level = (int)((t + add) >> qBits);
    du[blkPos] = (int)((t - ((long long)level << qBits)) >> (qBits - 8));
    sum += (uint32_t)level;
    const int sl = c < 0 ? -level : level;
    const int cl = sl < -32768 ? -32768 : sl > 32767 ? 32767 : sl;
    lev[blkPos] = cl;
    if (cl) top = sp >> 4;                                              // (sp ascends on a lane)
  }
  if (sum) QF_ADD_INTO(&ph->absSum, sum);
  if (top >= 0) QF_MAX_INTO(&ph->topSubset, top);
}

__device__ static inline void quant_flat_sbh(const QfUnit& u, const uint16_t* scan, const int32_t* src, int32_t* lev, const int32_t* du, uint32_t* abs_sum_out, const QfPhase* ph,
                                             const int lane, const int nlanes) {
  const int CGN = 1 << (2 * u.log2_size - 4);
  if (lane == 0) *abs_sum_out = ph->absSum;                             // (the sum before the hiding, as the reference reports it)
  if (!(u.sign_hide && ph->absSum >= 2)) return;
  const int topSubset = ph->topSubset;
  for (int subSet = lane; subSet <= topSubset && subSet < CGN; subSet += nlanes) {
    const uint16_t* sc = scan + (subSet << 4);
    const bool lastCG = subSet == topSubset;
    int firstNZ = 16, lastNZ = -1, sum = 0, n;
    for (n = 15; n >= 0; --n) if (lev[sc[n]]) { lastNZ = n; break; }
    for (n = 0; n < 16; n++) if (lev[sc[n]]) { firstNZ = n; break; }
    if (lastNZ - firstNZ < 4) continue;                                 // SBH_THRESHOLD
    for (n = firstNZ; n <= lastNZ; n++) sum += lev[sc[n]];
    const unsigned signbit = lev[sc[firstNZ]] > 0 ? 0 : 1;
    if (signbit == (unsigned)(sum & 1)) continue;
    int minCostInc = 0x7FFFFFFF, minPos = -1, finalChange = 0;
    for (n = lastCG ? lastNZ : 15; n >= 0; --n) {
      const int blkPos = sc[n];
      const int qv = lev[blkPos], d = du[blkPos];
      int curCost, curChange = 1;
      if (qv != 0) {
        if (d > 0) curCost = -d;
        else if (n == firstNZ && (qv == 1 || qv == -1)) curCost = 0x7FFFFFFF;      // a level of +-1 that opens the group is not lowered: the sign it carries would move
        else { curCost = d; curChange = -1; }
      } else if (n < firstNZ && (unsigned)(src[blkPos] >= 0 ? 0 : 1) != signbit) curCost = 0x7FFFFFFF;   // a new first level must carry the hidden sign
      else curCost = -d;
      if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minPos = blkPos; }
    }
    const int lm = lev[minPos];
    if (lm == 32767 || lm == -32768) finalChange = -1;
    lev[minPos] = src[minPos] >= 0 ? lm + finalChange : lm - finalChange;
  }
}
