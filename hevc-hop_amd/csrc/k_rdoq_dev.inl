// k_rdoq_dev.inl -- the device side of the rate-distortion optimised quantisation of one transform unit (see k_rdoq.hip), shared by k_rdoq (one lane per TU, 64 TUs
// per wave) and the fused leaf kernel of k_cabac.hip (one TU per workgroup).
#define RQ_SCAN_DIAG 0
#define RQ_SCAN_VER 2
#define RQ_C1FLAG_NUMBER 8
#define RQ_C2FLAG_NUMBER 1
#define RQ_COEF_REMAIN_BIN_REDUCTION 3
#define RQ_SBH_THRESHOLD 4
#define RQ_SCAN_SET_SIZE 16

// The quantiser scales (TComRom.cpp:164-172), g_uiGroupIdx (:353) and the 4x4 block's significance contexts are arithmetic on packed constants (hop_cabac_tab.h, each
// checked against its table at compile time): as __constant__ arrays indexed by a lane's register they were a vector-memory load per 4x4 position and two per non-zero
// level of the last-position pass, on the lane's dependent path.
#include "hop_cabac_tab.h"

// scan tables, built on the host (hop_rdoq_build_scans) and kept in device memory: scan[s][log2-2] at offset
// s*1360 + {0,16,80,336}; coefficient-group scans cg[s][log2-2] at 4080 + s*85 + {0,1,5,21}
__device__ static inline const uint16_t* rq_scan(const uint16_t* tabs, int s, int log2) {
  const int off = (log2 == 2) ? 0 : (log2 == 3) ? 16 : (log2 == 4) ? 80 : 336;
  return tabs + s * 1360 + off;
}
__device__ static inline const uint16_t* rq_scan_cg(const uint16_t* tabs, int s, int log2) {
  const int off = (log2 == 2) ? 0 : (log2 == 3) ? 1 : (log2 == 4) ? 5 : 21;
  return tabs + 4080 + s * 85 + off;
}

__device__ static inline int rq_ic_rate(const hop_estbits* eb, uint32_t absLevel, uint32_t ctxOne, uint32_t ctxAbs, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx) {
  int rate = 32768;                                                       // Int(xGetIEPRate())
  const uint32_t baseLevel = (c1Idx < RQ_C1FLAG_NUMBER) ? (2 + (c2Idx < RQ_C2FLAG_NUMBER)) : 1;
  if (absLevel >= baseLevel) {
    uint32_t symbol = absLevel - baseLevel, length;
    if (symbol < ((uint32_t)RQ_COEF_REMAIN_BIN_REDUCTION << goRice)) {
      length = symbol >> goRice;
      rate += (int)((length + 1 + goRice) << 15);
    } else {
      length = goRice;
      symbol = symbol - ((uint32_t)RQ_COEF_REMAIN_BIN_REDUCTION << goRice);
      while (symbol >= (1u << length)) symbol -= (1u << (length++));
      rate += (int)((RQ_COEF_REMAIN_BIN_REDUCTION + length + 1 - goRice + length) << 15);
    }
    if (c1Idx < RQ_C1FLAG_NUMBER) {
      rate += eb->greaterOneBits[ctxOne][1];
      if (c2Idx < RQ_C2FLAG_NUMBER) rate += eb->levelAbsBits[ctxAbs][1];
    }
  } else if (absLevel == 1) {
    rate += eb->greaterOneBits[ctxOne][0];
  } else if (absLevel == 2) {
    rate += eb->greaterOneBits[ctxOne][1];
    rate += eb->levelAbsBits[ctxAbs][0];
  } else {
    rate = 0;
  }
  return rate;
}

__device__ static inline uint32_t rq_coded_level(const hop_estbits* eb, double lambda, double& codedCost, double codedCost0, double& codedCostSig,
                                                 int levelDouble, uint32_t maxAbsLevel, uint32_t ctxSig, uint32_t ctxOne, uint32_t ctxAbs, uint32_t goRice,
                                                 uint32_t c1Idx, uint32_t c2Idx, int qBits, double dTemp, bool bLast) {
  double currCostSig = 0;
  uint32_t bestAbsLevel = 0;
  if (!bLast && maxAbsLevel < 3) {
    codedCostSig = lambda * (double)eb->significantBits[ctxSig][0];
    codedCost = codedCost0 + codedCostSig;
    if (maxAbsLevel == 0) return bestAbsLevel;
  } else {
    codedCost = 1.7e+308;                                                 // MAX_DOUBLE, CommonDef.h:121
  }
  if (!bLast) currCostSig = lambda * (double)eb->significantBits[ctxSig][1];
  const uint32_t minAbsLevel = (maxAbsLevel > 1 ? maxAbsLevel - 1 : 1);
  for (int absLevel = (int)maxAbsLevel; (uint32_t)absLevel >= minAbsLevel; absLevel--) {
    const double err = (double)(levelDouble - (int)((uint32_t)absLevel << qBits));
    double currCost = err * err * dTemp + lambda * (double)rq_ic_rate(eb, (uint32_t)absLevel, ctxOne, ctxAbs, goRice, c1Idx, c2Idx);
    currCost += currCostSig;
    if (currCost < codedCost) { bestAbsLevel = (uint32_t)absLevel; codedCost = currCost; codedCostSig = currCostSig; }
  }
  return bestAbsLevel;
}

// the coded_sub_block_flags of a TU are one 64-bit mask per lane (bit = raster index of the group, at most 8 x 8 groups)
__device__ static inline int rq_pattern_sig_ctx(unsigned long long cgFlag, uint32_t px, uint32_t py, int wcg) {
  if (wcg == 1) return -1;                                                // 4x4 block
  uint32_t r = 0, l = 0;
  if (px < (uint32_t)(wcg - 1)) r = (uint32_t)(cgFlag >> (py * wcg + px + 1)) & 1u;
  if (py < (uint32_t)(wcg - 1)) l = (uint32_t)(cgFlag >> ((py + 1) * wcg + px)) & 1u;
  return (int)(r + (l << 1));
}
__device__ static inline uint32_t rq_sig_cg_ctx(unsigned long long cgFlag, uint32_t px, uint32_t py, int wcg) {
  uint32_t r = 0, l = 0;
  if (px < (uint32_t)(wcg - 1)) r = (uint32_t)(cgFlag >> (py * wcg + px + 1)) & 1u;
  if (py < (uint32_t)(wcg - 1)) l = (uint32_t)(cgFlag >> ((py + 1) * wcg + px)) & 1u;
  return (r | l);
}
__device__ static inline int rq_sig_ctx_inc(int patternSigCtx, int scanIdx, int posX, int posY, int log2BlockSize, bool is_luma) {
  if (posX + posY == 0) return 0;
  if (log2BlockSize == 2) return hop_ctx_ind_map(4 * posY + posX);
  const int offset = log2BlockSize == 3 ? (scanIdx == RQ_SCAN_DIAG ? 9 : 15) : (is_luma ? 21 : 12);
  const int xs = posX & 3, ys = posY & 3;
  int cnt;
  if (patternSigCtx == 0) cnt = xs + ys <= 2 ? (xs + ys == 0 ? 2 : 1) : 0;
  else if (patternSigCtx == 1) cnt = ys <= 1 ? (ys == 0 ? 2 : 1) : 0;
  else if (patternSigCtx == 2) cnt = xs <= 1 ? (xs == 0 ? 2 : 1) : 0;
  else cnt = 2;
  return ((is_luma && ((posX >> 2) + (posY >> 2)) > 0) ? 3 : 0) + offset + cnt;
}
__device__ static inline double rq_rate_last(const hop_estbits* eb, double lambda, uint32_t posX, uint32_t posY) {
  const uint32_t ctxX = (uint32_t)hop_group_idx((int)posX), ctxY = (uint32_t)hop_group_idx((int)posY);
  double cost = (double)(eb->lastXBits[ctxX] + eb->lastYBits[ctxY]);
  if (ctxX > 3) cost += 32768.0 * (double)((ctxX - 2) >> 1);
  if (ctxY > 3) cost += 32768.0 * (double)((ctxY - 2) >> 1);
  return lambda * cost;
}

// bytes of per-coefficient state a lane keeps in the work area: cost of the chosen level and of its significance flag (double),
// level, |coeff| * Q, and the four sign-hiding terms (int)
#define RQ_WORK_PER_COEF 40

// One TU on the calling lane.  src / dst: its coefficients and levels; scan / scanCG: the TU's coefficient and coefficient-group scans; cgSig: CGN doubles `cgs` apart (the cost of each group's
// coded_sub_block_flag); wd: a work area of N2 * ws * RQ_WORK_PER_COEF bytes laid out [array][scan position][ws lanes], wl: the calling lane's column in it (ws = 64: the lanes of a
// wave side by side, k_rdoq; ws = 1: a TU of its own, k_turd_fused).  A lane only ever reads what it wrote itself: no barrier in here.
template <int LOG2>
__device__ static void rdoq_tu(const hop_rdoq_job& jb, const hop_estbits* __restrict__ eb, const uint16_t* __restrict__ scan, const uint16_t* __restrict__ scanCG,
                               double* __restrict__ cgSig, const int cgs, const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                               uint32_t* __restrict__ abs_sum_out, double* __restrict__ wd, const int ws, const int wl) {
  constexpr int N2 = 1 << (2 * LOG2), WCG = (1 << LOG2) >> 2, CGN = N2 >> 4;
  double* const wcc = wd + wl; double* const wcs = wd + (size_t)N2 * ws + wl;
  int* const wi = (int*)(wd + (size_t)2 * N2 * ws) + wl;
  int* const wlvl = wi; int* const wlvlD = wi + (size_t)N2 * ws; int* const wrUp = wi + (size_t)2 * N2 * ws;
  int* const wrDn = wi + (size_t)3 * N2 * ws; int* const wsDelta = wi + (size_t)4 * N2 * ws; int* const wdU = wi + (size_t)5 * N2 * ws;
#define W(a, sp) a[(size_t)(sp) * ws]
  const bool is_luma = jb.comp == 0;
  const int scan_idx = jb.scan_idx;
  const int per = jb.qp_scaled / 6, rem = jb.qp_scaled % 6;
  const int transformShift = 15 - jb.bit_depth - LOG2;                  // MAX_TR_DYNAMIC_RANGE - bitDepth - log2
  const int qBits = 14 + per + transformShift;                          // QUANT_SHIFT + per + shift
  const int q = hop_quant_scale(rem);
  const double errScale = ldexp((double)(1 << 15), -2 * transformShift);  // (1 << SCALE_BITS) * pow(2.0, -2.0*iTransformShift): exact
  const double dTemp = errScale / q / q / (1 << (2 * (jb.bit_depth - 8)));
  const double lambda = jb.lambda;
  const long long cap = (long long)0x7FFFFFFF - (1 << (qBits - 1));
  uint32_t absSum = 0;

  // ---- the level decision: one walk back along the scan, TComTrQuant.cpp:1574-1792 ----
  unsigned long long cgFlag = 0;
  uint32_t goRice = 0, ctxSet = 0, c1Idx = 0, c2Idx = 0;
  int c1 = 1, c2 = 0, lastScanPos = -1, cgLastScanPos = -1;
  double baseCost = 0, blockUncodedCost = 0;
  for (int cgScanPos = CGN - 1; cgScanPos >= 0; cgScanPos--) {
    const uint32_t cgBlkPos = scanCG[cgScanPos];
    const uint32_t cgPosY = cgBlkPos / WCG, cgPosX = cgBlkPos - cgPosY * WCG;
    int nnzBeforePos0 = 0; double codedLevelandDist = 0, uncodedDist = 0, sigCost = 0, sigCost0 = 0;
    const int patternSigCtx = rq_pattern_sig_ctx(cgFlag, cgPosX, cgPosY, WCG);
    uint32_t nzmask = 0;                                                // positions of this group whose chosen level is not zero
    cgSig[(size_t)cgScanPos * cgs] = 0;
    for (int scanPosinCG = 15; scanPosinCG >= 0; scanPosinCG--) {
      const int sp = cgScanPos * 16 + scanPosinCG;
      const uint32_t blkPos = scan[sp];
      // quantisation and the cost of coding nothing, :1545-1570
      int v = src[blkPos]; v = v < 0 ? -v : v;
      const long long t = (long long)v * q;
      const int levelDouble = (int)(t < cap ? t : cap);
      const uint32_t maxAbsLevel = (uint32_t)(levelDouble + (1 << (qBits - 1))) >> qBits;
      const double err0 = (double)levelDouble;
      const double cost0 = err0 * err0 * dTemp;
      W(wlvlD, sp) = levelDouble;
      blockUncodedCost += cost0;
      if (maxAbsLevel > 0 && lastScanPos < 0) {
        lastScanPos = sp;
        ctxSet = (sp < RQ_SCAN_SET_SIZE || !is_luma) ? 0 : 2;
        cgLastScanPos = cgScanPos;
      }
      double cc = 0, cs = 0;
      uint32_t level = 0;
      if (lastScanPos >= 0) {
        const uint32_t oneCtx = 4 * ctxSet + (uint32_t)c1, absCtx = ctxSet + (uint32_t)c2;
        int sDelta = 0;
        if (sp == lastScanPos) {
          level = rq_coded_level(eb, lambda, cc, cost0, cs, levelDouble, maxAbsLevel, 0, oneCtx, absCtx, goRice, c1Idx, c2Idx, qBits, dTemp, true);
        } else {
          const uint32_t posY = blkPos >> LOG2, posX = blkPos - (posY << LOG2);
          const uint32_t ctxSig = (uint32_t)rq_sig_ctx_inc(patternSigCtx, scan_idx, (int)posX, (int)posY, LOG2, is_luma);
          level = rq_coded_level(eb, lambda, cc, cost0, cs, levelDouble, maxAbsLevel, ctxSig, oneCtx, absCtx, goRice, c1Idx, c2Idx, qBits, dTemp, false);
          sDelta = eb->significantBits[ctxSig][1] - eb->significantBits[ctxSig][0];
        }
        W(wsDelta, sp) = sDelta;
        W(wdU, sp) = (levelDouble - (int)(level << qBits)) >> (qBits - 8);
        if (level > 0) {
          const int rateNow = rq_ic_rate(eb, level, oneCtx, absCtx, goRice, c1Idx, c2Idx);
          W(wrUp, sp) = rq_ic_rate(eb, level + 1, oneCtx, absCtx, goRice, c1Idx, c2Idx) - rateNow;
          W(wrDn, sp) = rq_ic_rate(eb, level - 1, oneCtx, absCtx, goRice, c1Idx, c2Idx) - rateNow;
        } else {
          W(wrUp, sp) = eb->greaterOneBits[oneCtx][0];
          W(wrDn, sp) = 0;
        }
        baseCost += cc;
        const uint32_t baseLevel = (c1Idx < RQ_C1FLAG_NUMBER) ? (2 + (c2Idx < RQ_C2FLAG_NUMBER)) : 1;
        if (level >= baseLevel) {
          if (level > 3u * (1u << goRice)) goRice = (goRice + 1 < 4u) ? goRice + 1 : 4u;
        }
        if (level >= 1) c1Idx++;
        if (level > 1) { c1 = 0; c2 += (c2 < 2); c2Idx++; }
        else if ((c1 < 3) && (c1 > 0) && level) c1++;
        if ((sp % RQ_SCAN_SET_SIZE == 0) && (sp > 0)) {
          c2 = 0; goRice = 0; c1Idx = 0; c2Idx = 0;
          ctxSet = (sp == RQ_SCAN_SET_SIZE || !is_luma) ? 0 : 2;
          if (c1 == 0) ctxSet++;
          c1 = 1;
        }
        W(wcc, sp) = cc; W(wcs, sp) = cs;
      } else {
        baseCost += cost0;
      }
      W(wlvl, sp) = (int)level;
      sigCost += cs;
      if (scanPosinCG == 0) sigCost0 = cs;
      if (level) {
        nzmask |= 1u << scanPosinCG;
        codedLevelandDist += cc - cs;
        uncodedDist += cost0;
        if (scanPosinCG != 0) nnzBeforePos0++;
      }
    }
    if (nzmask) cgFlag |= 1ull << cgBlkPos;
    if (cgLastScanPos >= 0) {
      if (cgScanPos) {
        if (!nzmask) {
          const uint32_t ctxSig = rq_sig_cg_ctx(cgFlag, cgPosX, cgPosY, WCG);
          baseCost += lambda * (double)eb->significantCoeffGroupBits[ctxSig][0] - sigCost;
          cgSig[(size_t)cgScanPos * cgs] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
        } else if (cgScanPos < cgLastScanPos) {
          if (nnzBeforePos0 == 0) { baseCost -= sigCost0; sigCost -= sigCost0; }
          double costZeroCG = baseCost;
          const uint32_t ctxSig = rq_sig_cg_ctx(cgFlag, cgPosX, cgPosY, WCG);
          baseCost += lambda * (double)eb->significantCoeffGroupBits[ctxSig][1];
          costZeroCG += lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
          cgSig[(size_t)cgScanPos * cgs] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][1];
          costZeroCG += uncodedDist;
          costZeroCG -= codedLevelandDist;
          costZeroCG -= sigCost;
          if (costZeroCG < baseCost) {
            cgFlag &= ~(1ull << cgBlkPos);
            baseCost = costZeroCG;
            cgSig[(size_t)cgScanPos * cgs] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
            for (int p = 15; p >= 0; p--) {
              if (!((nzmask >> p) & 1u)) continue;
              const int sp = cgScanPos * 16 + p;
              const double e = (double)W(wlvlD, sp);
              W(wlvl, sp) = 0; W(wcc, sp) = e * e * dTemp; W(wcs, sp) = 0;
            }
          }
        }
      } else {
        cgFlag |= 1ull << cgBlkPos;
      }
    }
  }
  // ---- the last position, :1794-1866 ----
  int bestLastIdxP1 = 0;
  if (lastScanPos >= 0) {
    double bestCost;
    if (!jb.is_intra && is_luma && jb.tr_depth == 0) {
      bestCost = blockUncodedCost + lambda * (double)eb->blockRootCbpBits[0][0];
      baseCost += lambda * (double)eb->blockRootCbpBits[0][1];
    } else {
      int ctxCbf = is_luma ? (jb.tr_depth == 0 ? 1 : 0) : jb.tr_depth;          // getCtxQtCbf, TComDataCU.cpp:1848-1859
      ctxCbf = (is_luma ? 0 : 1) * 4 + ctxCbf;                                    // NUM_QT_CBF_CTX
      bestCost = blockUncodedCost + lambda * (double)eb->blockCbpBits[ctxCbf][0];
      baseCost += lambda * (double)eb->blockCbpBits[ctxCbf][1];
    }
    bool foundLast = false;
    for (int cgScanPos = cgLastScanPos; cgScanPos >= 0 && !foundLast; cgScanPos--) {
      const uint32_t cgBlkPos = scanCG[cgScanPos];
      baseCost -= cgSig[(size_t)cgScanPos * cgs];
      if ((cgFlag >> cgBlkPos) & 1ull) {
        for (int p = 15; p >= 0; p--) {
          const int sp = cgScanPos * 16 + p;
          if (sp > lastScanPos) continue;
          const int lv = W(wlvl, sp);
          if (lv) {
            const uint32_t blkPos = scan[sp];
            const uint32_t posY = blkPos >> LOG2, posX = blkPos - (posY << LOG2);
            const double costLast = scan_idx == RQ_SCAN_VER ? rq_rate_last(eb, lambda, posY, posX) : rq_rate_last(eb, lambda, posX, posY);
            const double totalCost = baseCost + costLast - W(wcs, sp);
            if (totalCost < bestCost) { bestLastIdxP1 = sp + 1; bestCost = totalCost; }
            if (lv > 1) { foundLast = true; break; }
            const double e = (double)W(wlvlD, sp);
            baseCost -= W(wcc, sp);
            baseCost += e * e * dTemp;
          } else {
            baseCost -= W(wcs, sp);
          }
        }
      }
    }
    for (int sp = 0; sp < bestLastIdxP1; sp++) {
      const int level = W(wlvl, sp);
      if (level) {
        absSum += (uint32_t)level;
        if (src[scan[sp]] < 0) W(wlvl, sp) = -level;
      }
    }
    for (int sp = bestLastIdxP1; sp <= lastScanPos; sp++) W(wlvl, sp) = 0;
  }
  // ---- sign bit hiding, :1883-1998 ----
  if (lastScanPos >= 0 && jb.sign_hide && absSum >= 2) {
    // Int arithmetic in the reference: inv*inv*(1<<(2*per)) wraps for per >= 10; reproduced as wrapping 32-bit
    const int32_t prod = (int32_t)((uint32_t)(hop_inv_quant_scale(rem) * hop_inv_quant_scale(rem)) * (uint32_t)(1u << ((2 * per) & 31)));
    const long long rdFactor = (long long)((double)prod / lambda / 16 / (1 << (2 * (jb.bit_depth - 8))) + 0.5);
    int lastCG = -1;
    for (int subSet = lastScanPos >> 4; subSet >= 0; subSet--) {        // the groups above hold no level
      const int subPos = subSet << 4;
      int firstNZ = RQ_SCAN_SET_SIZE, lastNZ = -1, sum = 0, n;
      for (n = RQ_SCAN_SET_SIZE - 1; n >= 0; --n) if (W(wlvl, n + subPos)) { lastNZ = n; break; }
      for (n = 0; n < RQ_SCAN_SET_SIZE; n++) if (W(wlvl, n + subPos)) { firstNZ = n; break; }
      for (n = firstNZ; n <= lastNZ; n++) sum += W(wlvl, n + subPos);
      if (lastNZ >= 0 && lastCG == -1) lastCG = 1;
      if (lastNZ - firstNZ >= RQ_SBH_THRESHOLD) {
        const uint32_t signbit = (W(wlvl, subPos + firstNZ) > 0 ? 0 : 1);
        if (signbit != (uint32_t)(sum & 0x1)) {
          long long minCostInc = 0x7FFFFFFFFFFFFFFFLL, curCost = 0x7FFFFFFFFFFFFFFFLL;
          int minPos = -1, finalChange = 0, curChange = 0;
          for (n = (lastCG == 1 ? lastNZ : RQ_SCAN_SET_SIZE - 1); n >= 0; --n) {
            const int sp = n + subPos;
            const int lv = W(wlvl, sp), alv = lv < 0 ? -lv : lv;
            const int du = W(wdU, sp);
            if (lv != 0) {
              const long long costUp = rdFactor * (-du) + W(wrUp, sp);
              long long costDown = rdFactor * (du) + W(wrDn, sp) - ((alv == 1) ? W(wsDelta, sp) : 0);
              if (lastCG == 1 && lastNZ == n && alv == 1) costDown -= (4 << 15);
              if (costUp < costDown) { curCost = costUp; curChange = 1; }
              else {
                curChange = -1;
                if (n == firstNZ && alv == 1) curCost = 0x7FFFFFFFFFFFFFFFLL; else curCost = costDown;
              }
            } else {
              curCost = rdFactor * (-(du < 0 ? -du : du)) + (1 << 15) + W(wrUp, sp) + W(wsDelta, sp);
              curChange = 1;
              if (n < firstNZ) {
                const uint32_t thissignbit = (src[scan[sp]] >= 0 ? 0 : 1);
                if (thissignbit != signbit) curCost = 0x7FFFFFFFFFFFFFFFLL;
              }
            }
            if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minPos = sp; }
          }
          const int lm = W(wlvl, minPos);
          if (lm == 32767 || lm == -32768) finalChange = -1;
          W(wlvl, minPos) = (src[scan[minPos]] >= 0) ? lm + finalChange : lm - finalChange;
        }
      }
      if (lastCG == 1) lastCG = 0;
    }
  }
  *abs_sum_out = absSum;
  for (int sp = 0; sp < N2; sp++) dst[scan[sp]] = (sp <= lastScanPos) ? W(wlvl, sp) : 0;
#undef W
}

// ---- The phased form: the same unit, the same bytes in dst / abs_sum, for a unit that has lanes to itself (the fused leaf bodies of k_leaf_fused.inl). ----
// rdoq_tu does three kinds of work on its one lane.  Only one of them is a recurrence: the level decision at and below the last significant position, whose context set,
// c1 / c2, Rice parameter and running cost each depend on the decision before.  The rest depends on the position alone -- quantisation, the cost of coding nothing, the
// significance context of each of the four neighbour patterns, where the last significant position is; and, after the decisions, the signs, sign-bit hiding (a 16-position
// subset reads and writes only its own levels) and the scatter into raster order.  Here those are functions of (lane, nlanes), a position / group / subset per lane and step:
//   rdoq_prep_pos | rdoq_prep_groups | rdoq_serial<LOG2> (ONE lane) | rdoq_finish_levels | rdoq_finish_sbh | rdoq_finish_scatter
// `|` is a barrier of the lanes that serve the unit, with the memory between them made visible (the work area of a 32x32 unit is HBM).  The barrier is the caller's: none
// of the functions holds one, so each may stand under a condition that is uniform over those lanes.  The work area is rdoq_tu's at ws = 1 (N2 * RQ_WORK_PER_COEF bytes).
// The prepared values -- |coefficient| * Q, the cost of coding nothing, the four significance contexts -- go where RqPrep points: arrays of their own (the workgroup
// body: in LDS whatever the unit's size, because the serial lane's reads of them are on its dependent path and a 32x32 unit's work area is HBM), or rq_prep_in_work: three
// arrays of the work area itself (wlvlD, wcc, wsDelta), the last two of which carry the prepared value until the serial lane replaces it with its own.
// Doubles are computed by rdoq_tu's own expressions and summed in its order (-ffp-contract=off: the lane an expression runs on does not change its rounding); everything a
// reduction over lanes combines is an integer.  host/hop_rdoq_host.cpp builds both forms for the host; tests/test_rdoq_phased_cpu.py compares them.
struct RqPhase { int lastScanPos, bestLastIdxP1, topSubset; uint32_t absSum; };   // what the phases hand on (LDS in the leaf bodies); rdoq_prep_pos initialises it
#if defined(RQ_HOST)
#define RQ_MAX_INTO(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)  // (emulated lanes run one after the other)
#define RQ_ADD_INTO(p, v) (*(p) += (v))
#else
#define RQ_MAX_INTO(p, v) atomicMax((p), (v))
#define RQ_ADD_INTO(p, v) atomicAdd((p), (v))
#endif
struct RqQuant { int qBits, q; double dTemp; long long cap; };
__device__ static inline RqQuant rq_quant(const hop_rdoq_job& jb) {    // rdoq_tu's constants, by its expressions
  const int LOG2 = jb.log2_size;
  const int per = jb.qp_scaled / 6, rem = jb.qp_scaled % 6;
  const int transformShift = 15 - jb.bit_depth - LOG2;
  RqQuant k;
  k.qBits = 14 + per + transformShift;
  k.q = hop_quant_scale(rem);
  const double errScale = ldexp((double)(1 << 15), -2 * transformShift);
  k.dTemp = errScale / k.q / k.q / (1 << (2 * (jb.bit_depth - 8)));
  k.cap = (long long)0x7FFFFFFF - (1 << (k.qBits - 1));
  return k;
}
struct RqPrep { int* lvlD; double* cost0; int* ctx; };
#define RQW(N2) double* const wcc = wd; double* const wcs = wd + (N2); int* const wlvl = (int*)(wd + 2 * (N2)); int* const wlvlD = wlvl + (N2); int* const wrUp = wlvl + 2 * (N2); \
                int* const wrDn = wlvl + 3 * (N2); int* const wsDelta = wlvl + 4 * (N2); int* const wdU = wlvl + 5 * (N2); \
                (void)wcc; (void)wcs; (void)wlvlD; (void)wrUp; (void)wrDn; (void)wsDelta; (void)wdU

__device__ static inline RqPrep rq_prep_in_work(double* wd, const int N2) { RQW(N2); RqPrep pp; pp.lvlD = wlvlD; pp.cost0 = wcc; pp.ctx = wsDelta; (void)wlvl; return pp; }
// every scan position: |coefficient| * Q, the cost of coding nothing, the significance context under each neighbour pattern, a byte each
__device__ static inline void rdoq_prep_pos(const hop_rdoq_job& jb, const uint16_t* scan, const int32_t* src, const RqPrep pp, RqPhase* ph, const int lane, const int nlanes) {
  const int LOG2 = jb.log2_size, N2 = 1 << (2 * LOG2);
  const RqQuant k = rq_quant(jb);
  const bool is_luma = jb.comp == 0;
  if (lane == 0) { ph->lastScanPos = -1; ph->bestLastIdxP1 = 0; ph->topSubset = -1; ph->absSum = 0; }
  for (int sp = lane; sp < N2; sp += nlanes) {
    const uint32_t blkPos = scan[sp];
    int v = src[blkPos]; v = v < 0 ? -v : v;
    const long long t = (long long)v * k.q;
    const int levelDouble = (int)(t < k.cap ? t : k.cap);
    const double err0 = (double)levelDouble;
    const double cost0 = err0 * err0 * k.dTemp;
    pp.lvlD[sp] = levelDouble;
    pp.cost0[sp] = cost0;
    const int posY = (int)(blkPos >> LOG2), posX = (int)(blkPos - ((uint32_t)posY << LOG2));
    uint32_t word = 0;
    for (int pat = 0; pat < 4; pat++) word |= (uint32_t)rq_sig_ctx_inc(pat, jb.scan_idx, posX, posY, LOG2, is_luma) << (8 * pat);
    pp.ctx[sp] = (int)word;
  }
}
// every coefficient group: which of its positions have a candidate level above zero (cgMask); the last such position of the unit (ph->lastScanPos, a maximum over lanes)
__device__ static inline void rdoq_prep_groups(const hop_rdoq_job& jb, uint16_t* cgMask, const RqPrep pp, RqPhase* ph, const int lane, const int nlanes) {
  const int N2 = 1 << (2 * jb.log2_size), CGN = N2 >> 4;
  const RqQuant k = rq_quant(jb);
  for (int cg = lane; cg < CGN; cg += nlanes) {
    uint32_t mask = 0;
    for (int p = 0; p < 16; p++) if (((uint32_t)(pp.lvlD[cg * 16 + p] + (1 << (k.qBits - 1))) >> k.qBits) > 0) mask |= 1u << p;
    cgMask[cg] = (uint16_t)mask;
    if (mask) RQ_MAX_INTO(&ph->lastScanPos, cg * 16 + 31 - __builtin_clz(mask));
  }
}

// rq_coded_level, which also hands out the rates it computed: rMax of maxAbsLevel, rM1 of maxAbsLevel - 1 (set where the loop of rq_coded_level reaches that level)
__device__ static inline uint32_t rq_coded_level_r(const hop_estbits* eb, double lambda, double& codedCost, double codedCost0, double& codedCostSig,
                                                   int levelDouble, uint32_t maxAbsLevel, uint32_t ctxSig, uint32_t ctxOne, uint32_t ctxAbs, uint32_t goRice,
                                                   uint32_t c1Idx, uint32_t c2Idx, int qBits, double dTemp, bool bLast, int& rMax, int& rM1) {
  double currCostSig = 0;
  uint32_t bestAbsLevel = 0;
  if (!bLast && maxAbsLevel < 3) {
    codedCostSig = lambda * (double)eb->significantBits[ctxSig][0];
    codedCost = codedCost0 + codedCostSig;
    if (maxAbsLevel == 0) return bestAbsLevel;
  } else {
    codedCost = 1.7e+308;                                                 // MAX_DOUBLE, CommonDef.h:121
  }
  if (!bLast) currCostSig = lambda * (double)eb->significantBits[ctxSig][1];
  const uint32_t minAbsLevel = (maxAbsLevel > 1 ? maxAbsLevel - 1 : 1);
  for (int absLevel = (int)maxAbsLevel; (uint32_t)absLevel >= minAbsLevel; absLevel--) {
    const double err = (double)(levelDouble - (int)((uint32_t)absLevel << qBits));
    const int rate = rq_ic_rate(eb, (uint32_t)absLevel, ctxOne, ctxAbs, goRice, c1Idx, c2Idx);
    if ((uint32_t)absLevel == maxAbsLevel) rMax = rate; else rM1 = rate;
    double currCost = err * err * dTemp + lambda * (double)rate;
    currCost += currCostSig;
    if (currCost < codedCost) { bestAbsLevel = (uint32_t)absLevel; codedCost = currCost; codedCostSig = currCostSig; }
  }
  return bestAbsLevel;
}

// ONE lane: the level decision from the last significant position down, the group decisions, the last position (rdoq_tu's loops in its order and arithmetic, TComTrQuant.cpp:1574-1866).
// Above the last significant position rdoq_tu adds the same cost0 to blockUncodedCost and to baseCost, both from zero and in the same order: one sum, copied at the boundary.
// Leaves: wlvl (levels without sign) and the sign-hiding terms for every position at or below ph->lastScanPos, ph->bestLastIdxP1.
template <int LOG2>
__device__ static void rdoq_serial(const hop_rdoq_job& jb, const hop_estbits* __restrict__ eb, const uint16_t* __restrict__ scan, const uint16_t* __restrict__ scanCG,
                                   double* __restrict__ cgSig, const uint16_t* __restrict__ cgMask, RqPhase* ph, double* wd, const RqPrep pp) {
  constexpr int N2 = 1 << (2 * LOG2), WCG = (1 << LOG2) >> 2;
  RQW(N2);
  const int lastScanPos = ph->lastScanPos;
  if (lastScanPos < 0) return;                                            // no level anywhere: nothing below reads a cost (ph->bestLastIdxP1 is 0)
  const bool is_luma = jb.comp == 0;
  const int scan_idx = jb.scan_idx;
  const RqQuant k = rq_quant(jb);
  const int qBits = k.qBits;
  const double dTemp = k.dTemp, lambda = jb.lambda;
  const int cgLastScanPos = lastScanPos >> 4;
  double blockUncodedCost = 0;
  for (int sp = N2 - 1; sp > lastScanPos; sp--) blockUncodedCost += pp.cost0[sp];
  double baseCost = blockUncodedCost;
  unsigned long long cgFlag = 0;
  uint32_t goRice = 0, ctxSet = (lastScanPos < RQ_SCAN_SET_SIZE || !is_luma) ? 0 : 2, c1Idx = 0, c2Idx = 0;
  int c1 = 1, c2 = 0;
  for (int cgScanPos = cgLastScanPos; cgScanPos >= 0; cgScanPos--) {
    const uint32_t cgBlkPos = scanCG[cgScanPos];
    const uint32_t cgPosY = cgBlkPos / WCG, cgPosX = cgBlkPos - cgPosY * WCG;
    int nnzBeforePos0 = 0; double codedLevelandDist = 0, uncodedDist = 0, sigCost = 0, sigCost0 = 0;
    const int patternSigCtx = rq_pattern_sig_ctx(cgFlag, cgPosX, cgPosY, WCG);
    const int patShift = 8 * (patternSigCtx & 3);                        // (a 4x4 unit has no pattern: its four bytes are the same)
    const uint32_t cand = cgMask[cgScanPos];                            // positions of this group whose candidate level is not zero
    uint32_t nzmask = 0;                                                // positions of this group whose chosen level is not zero
    cgSig[cgScanPos] = 0;
    for (int scanPosinCG = (cgScanPos == cgLastScanPos) ? (lastScanPos & 15) : 15; scanPosinCG >= 0; scanPosinCG--) {
      const int sp = cgScanPos * 16 + scanPosinCG;
      const int levelDouble = pp.lvlD[sp];
      const double cost0 = pp.cost0[sp];
      const uint32_t maxAbsLevel = ((cand >> scanPosinCG) & 1u) ? (uint32_t)(levelDouble + (1 << (qBits - 1))) >> qBits : 0u;
      blockUncodedCost += cost0;
      double cc = 0, cs = 0;
      uint32_t level = 0;
      const uint32_t oneCtx = 4 * ctxSet + (uint32_t)c1, absCtx = ctxSet + (uint32_t)c2;
      int sDelta = 0, rMax = 0, rM1 = 0;
      if (sp == lastScanPos) {
        level = rq_coded_level_r(eb, lambda, cc, cost0, cs, levelDouble, maxAbsLevel, 0, oneCtx, absCtx, goRice, c1Idx, c2Idx, qBits, dTemp, true, rMax, rM1);
      } else {
        const uint32_t ctxSig = ((uint32_t)pp.ctx[sp] >> patShift) & 0xFFu;
        level = rq_coded_level_r(eb, lambda, cc, cost0, cs, levelDouble, maxAbsLevel, ctxSig, oneCtx, absCtx, goRice, c1Idx, c2Idx, qBits, dTemp, false, rMax, rM1);
        sDelta = eb->significantBits[ctxSig][1] - eb->significantBits[ctxSig][0];
      }
      wsDelta[sp] = sDelta;
      wdU[sp] = (levelDouble - (int)(level << qBits)) >> (qBits - 8);
      if (level > 0) {
        // the rates of the chosen level and of its neighbours: rq_ic_rate is a function of its arguments, and rq_coded_level_r has evaluated it at maxAbsLevel and,
        // where maxAbsLevel > 1, at maxAbsLevel - 1 with these very arguments
        const bool atMax = level == maxAbsLevel;
        const int rateNow = atMax ? rMax : rM1;
        const int rateUp = atMax ? rq_ic_rate(eb, level + 1, oneCtx, absCtx, goRice, c1Idx, c2Idx) : rMax;
        const int rateDn = (atMax && maxAbsLevel > 1) ? rM1 : rq_ic_rate(eb, level - 1, oneCtx, absCtx, goRice, c1Idx, c2Idx);
        wrUp[sp] = rateUp - rateNow;
        wrDn[sp] = rateDn - rateNow;
      } else {
        wrUp[sp] = eb->greaterOneBits[oneCtx][0];
        wrDn[sp] = 0;
      }
      baseCost += cc;
      const uint32_t baseLevel = (c1Idx < RQ_C1FLAG_NUMBER) ? (2 + (c2Idx < RQ_C2FLAG_NUMBER)) : 1;
      if (level >= baseLevel) {
        if (level > 3u * (1u << goRice)) goRice = (goRice + 1 < 4u) ? goRice + 1 : 4u;
      }
      if (level >= 1) c1Idx++;
      if (level > 1) { c1 = 0; c2 += (c2 < 2); c2Idx++; }
      else if ((c1 < 3) && (c1 > 0) && level) c1++;
      if ((sp % RQ_SCAN_SET_SIZE == 0) && (sp > 0)) {
        c2 = 0; goRice = 0; c1Idx = 0; c2Idx = 0;
        ctxSet = (sp == RQ_SCAN_SET_SIZE || !is_luma) ? 0 : 2;
        if (c1 == 0) ctxSet++;
        c1 = 1;
      }
      wcc[sp] = cc; wcs[sp] = cs;
      wlvl[sp] = (int)level;
      sigCost += cs;
      if (scanPosinCG == 0) sigCost0 = cs;
      if (level) {
        nzmask |= 1u << scanPosinCG;
        codedLevelandDist += cc - cs;
        uncodedDist += cost0;
        if (scanPosinCG != 0) nnzBeforePos0++;
      }
    }
    if (nzmask) cgFlag |= 1ull << cgBlkPos;
    if (cgScanPos) {
      if (!nzmask) {
        const uint32_t ctxSig = rq_sig_cg_ctx(cgFlag, cgPosX, cgPosY, WCG);
        baseCost += lambda * (double)eb->significantCoeffGroupBits[ctxSig][0] - sigCost;
        cgSig[cgScanPos] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
      } else if (cgScanPos < cgLastScanPos) {
        if (nnzBeforePos0 == 0) { baseCost -= sigCost0; sigCost -= sigCost0; }
        double costZeroCG = baseCost;
        const uint32_t ctxSig = rq_sig_cg_ctx(cgFlag, cgPosX, cgPosY, WCG);
        baseCost += lambda * (double)eb->significantCoeffGroupBits[ctxSig][1];
        costZeroCG += lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
        cgSig[cgScanPos] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][1];
        costZeroCG += uncodedDist;
        costZeroCG -= codedLevelandDist;
        costZeroCG -= sigCost;
        if (costZeroCG < baseCost) {
          cgFlag &= ~(1ull << cgBlkPos);
          baseCost = costZeroCG;
          cgSig[cgScanPos] = lambda * (double)eb->significantCoeffGroupBits[ctxSig][0];
          for (int p = 15; p >= 0; p--) {
            if (!((nzmask >> p) & 1u)) continue;
            const int sp = cgScanPos * 16 + p;
            const double e = (double)pp.lvlD[sp];
            wlvl[sp] = 0; wcc[sp] = e * e * dTemp; wcs[sp] = 0;
          }
        }
      }
    } else {
      cgFlag |= 1ull << cgBlkPos;
    }
  }
  // ---- the last position, :1794-1866 ----
  int bestLastIdxP1 = 0;
  double bestCost;
  if (!jb.is_intra && is_luma && jb.tr_depth == 0) {
    bestCost = blockUncodedCost + lambda * (double)eb->blockRootCbpBits[0][0];
    baseCost += lambda * (double)eb->blockRootCbpBits[0][1];
  } else {
    int ctxCbf = is_luma ? (jb.tr_depth == 0 ? 1 : 0) : jb.tr_depth;          // getCtxQtCbf, TComDataCU.cpp:1848-1859
    ctxCbf = (is_luma ? 0 : 1) * 4 + ctxCbf;                                    // NUM_QT_CBF_CTX
    bestCost = blockUncodedCost + lambda * (double)eb->blockCbpBits[ctxCbf][0];
    baseCost += lambda * (double)eb->blockCbpBits[ctxCbf][1];
  }
  bool foundLast = false;
  for (int cgScanPos = cgLastScanPos; cgScanPos >= 0 && !foundLast; cgScanPos--) {
    const uint32_t cgBlkPos = scanCG[cgScanPos];
    baseCost -= cgSig[cgScanPos];
    if ((cgFlag >> cgBlkPos) & 1ull) {
      for (int p = 15; p >= 0; p--) {
        const int sp = cgScanPos * 16 + p;
        if (sp > lastScanPos) continue;
        const int lv = wlvl[sp];
        if (lv) {
          const uint32_t blkPos = scan[sp];
          const uint32_t posY = blkPos >> LOG2, posX = blkPos - (posY << LOG2);
          const double costLast = scan_idx == RQ_SCAN_VER ? rq_rate_last(eb, lambda, posY, posX) : rq_rate_last(eb, lambda, posX, posY);
          const double totalCost = baseCost + costLast - wcs[sp];
          if (totalCost < bestCost) { bestLastIdxP1 = sp + 1; bestCost = totalCost; }
          if (lv > 1) { foundLast = true; break; }
          const double e = (double)pp.lvlD[sp];
          baseCost -= wcc[sp];
          baseCost += e * e * dTemp;
        } else {
          baseCost -= wcs[sp];
        }
      }
    }
  }
  ph->bestLastIdxP1 = bestLastIdxP1;
}

// every position at or below the last significant one: the sign, zero from the chosen last position on; the sum of the levels and the highest 16-position subset that
// keeps one (an integer sum and a maximum over lanes: any order)
__device__ static inline void rdoq_finish_levels(const hop_rdoq_job& jb, const uint16_t* scan, const int32_t* src, double* wd, RqPhase* ph, const int lane, const int nlanes) {
  const int N2 = 1 << (2 * jb.log2_size);
  RQW(N2);
  const int lastScanPos = ph->lastScanPos, bestLastIdxP1 = ph->bestLastIdxP1;
  uint32_t sum = 0; int top = -1;
  // (up to the end of the last significant position's subset: sign hiding looks for levels in all sixteen, and the serial lane has written none above that position)
  for (int sp = lane; sp <= (lastScanPos | 15); sp += nlanes) {
    if (sp < bestLastIdxP1) {
      const int level = wlvl[sp];
      if (level) {
        sum += (uint32_t)level;
        if ((sp >> 4) > top) top = sp >> 4;
        if (src[scan[sp]] < 0) wlvl[sp] = -level;
      }
    } else wlvl[sp] = 0;
  }
  if (sum) RQ_ADD_INTO(&ph->absSum, sum);
  if (top >= 0) RQ_MAX_INTO(&ph->topSubset, top);
}
// sign bit hiding (:1883-1998), a 16-position subset per lane and step.  rdoq_tu walks the subsets downwards and treats the first one that holds a level as the last
// group (lastCG == 1); a subset without a level is never changed, so that subset is the highest one holding a level before any change: ph->topSubset.
__device__ static inline void rdoq_finish_sbh(const hop_rdoq_job& jb, const uint16_t* scan, const int32_t* src, double* wd, RqPhase* ph, const int lane, const int nlanes) {
  const int N2 = 1 << (2 * jb.log2_size);
  RQW(N2);
  const int lastScanPos = ph->lastScanPos;
  if (!(lastScanPos >= 0 && jb.sign_hide && ph->absSum >= 2)) return;
  const int per = jb.qp_scaled / 6, rem = jb.qp_scaled % 6;
  // Int arithmetic in the reference: inv*inv*(1<<(2*per)) wraps for per >= 10; reproduced as wrapping 32-bit
  const int32_t prod = (int32_t)((uint32_t)(hop_inv_quant_scale(rem) * hop_inv_quant_scale(rem)) * (uint32_t)(1u << ((2 * per) & 31)));
  const long long rdFactor = (long long)((double)prod / jb.lambda / 16 / (1 << (2 * (jb.bit_depth - 8))) + 0.5);
  const int topSubset = ph->topSubset;
  for (int subSet = lane; subSet <= (lastScanPos >> 4); subSet += nlanes) {
    const int subPos = subSet << 4;
    const bool lastCG = subSet == topSubset;
    int firstNZ = RQ_SCAN_SET_SIZE, lastNZ = -1, sum = 0, n;
    for (n = RQ_SCAN_SET_SIZE - 1; n >= 0; --n) if (wlvl[n + subPos]) { lastNZ = n; break; }
    for (n = 0; n < RQ_SCAN_SET_SIZE; n++) if (wlvl[n + subPos]) { firstNZ = n; break; }
    for (n = firstNZ; n <= lastNZ; n++) sum += wlvl[n + subPos];
    if (lastNZ - firstNZ < RQ_SBH_THRESHOLD) continue;
    const uint32_t signbit = (wlvl[subPos + firstNZ] > 0 ? 0 : 1);
    if (signbit == (uint32_t)(sum & 0x1)) continue;
    long long minCostInc = 0x7FFFFFFFFFFFFFFFLL, curCost = 0x7FFFFFFFFFFFFFFFLL;
    int minPos = -1, finalChange = 0, curChange = 0;
    for (n = (lastCG ? lastNZ : RQ_SCAN_SET_SIZE - 1); n >= 0; --n) {
      const int sp = n + subPos;
      const int lv = wlvl[sp], alv = lv < 0 ? -lv : lv;
      const int du = wdU[sp];
      if (lv != 0) {
        const long long costUp = rdFactor * (-du) + wrUp[sp];
        long long costDown = rdFactor * (du) + wrDn[sp] - ((alv == 1) ? wsDelta[sp] : 0);
        if (lastCG && lastNZ == n && alv == 1) costDown -= (4 << 15);
        if (costUp < costDown) { curCost = costUp; curChange = 1; }
        else {
          curChange = -1;
          if (n == firstNZ && alv == 1) curCost = 0x7FFFFFFFFFFFFFFFLL; else curCost = costDown;
        }
      } else {
        curCost = rdFactor * (-(du < 0 ? -du : du)) + (1 << 15) + wrUp[sp] + wsDelta[sp];
        curChange = 1;
        if (n < firstNZ) {
          const uint32_t thissignbit = (src[scan[sp]] >= 0 ? 0 : 1);
          if (thissignbit != signbit) curCost = 0x7FFFFFFFFFFFFFFFLL;
        }
      }
      if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minPos = sp; }
    }
    const int lm = wlvl[minPos];
    if (lm == 32767 || lm == -32768) finalChange = -1;
    wlvl[minPos] = (src[scan[minPos]] >= 0) ? lm + finalChange : lm - finalChange;
  }
}
// the levels into raster order, zero above the last significant position; the sum
__device__ static inline void rdoq_finish_scatter(const hop_rdoq_job& jb, const uint16_t* scan, int32_t* dst, uint32_t* abs_sum_out, double* wd, RqPhase* ph, const int lane,
                                                  const int nlanes) {
  const int N2 = 1 << (2 * jb.log2_size);
  RQW(N2);
  const int lastScanPos = ph->lastScanPos;
  if (lane == 0) *abs_sum_out = ph->absSum;
  for (int sp = lane; sp < N2; sp += nlanes) dst[scan[sp]] = (sp <= lastScanPos) ? wlvl[sp] : 0;
}

