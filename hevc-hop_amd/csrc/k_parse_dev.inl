// k_parse_dev.inl -- the slice data of a picture read back: the arithmetic decoder, the CTU loop of TDecSlice::decompressSlice and the TDecSbac parsers behind it, with
// everything a decoder derives instead of reading (intra directions, merge and AMVP motion).  The mirror image of k_entropy_dev.inl, written once and compiled twice: for
// the device by csrc/k_parse.hip (hop_slice_data_parse) and for the host by host/hop_parse.cpp (hop_slice_data_parse_host, the yardstick).
// The including file defines ENT_FN / ENT_TAB and has included k_entropy_dev.inl: the context-set layout (EN_*), the CABAC tables, the scan helpers, en_part, en_mpm,
// en_intra_scan and en_cbf_ctx are the writer's, so that the two bodies cannot drift apart.
//
// Replaces (paths under source/Lib of the reference):
//   TDecBinCABAC TLibDecoder/TDecBinCoderCABAC.cpp: start :65, finish :75, decodeBin :100, decodeBinEP :146, decodeBinsEP :165, decodeBinTrm :212, over a byte cursor
//   with a hard end (TComInputBitstream::readByte);
//   the CTU loop of TDecSlice::decompressSlice TDecSlice.cpp:108-380 (SAO parameters :312-345, decodeCU :350, the WaveFrontSynchro load / store :196-262, :371, the
//   end_of_substream bin :358-366), TDecCu::decodeCU / xDecodeCU / xFinishDecodeCU / xDecodeSliceEnd TDecCu.cpp:122-380, TDecEntropy::decodePUWise :160-287,
//   decodeMVPIdxPU :363-433, xDecodeTransform :453-646, decodeCoeff :665-693 (TDecEntropy.cpp), the TDecSbac parsers (TDecSbac.cpp: parseSplitFlag :544, parseSkipFlag
//   :425, parsePredMode :652, parsePartSize :571, parseMergeFlag / Index :464 / :497, parseGTFlag :484, parseMvd :838, parseGT :903 with the fourth corner of the affine
//   form :1329-1337, parseMVPIdx :533, parseIntraDirLumaAng :670, parseIntraDirChroma :735, parseQtRootCbf :1370, parseQtCbf :1428, parseTransformSubdivFlag :1356,
//   parseTransformSkipFlags :1449, parseLastSignificantXY :1497, parseCoeffNxN :1556-1830, xReadCoefRemainExGolomb, xReadEpExGolomb, parseSAOBlkParam :1906 with
//   :1835-1901), and what the decoder derives: TComDataCU::getIntraDirLumaPredictor (en_mpm), getAllowedChromaDir, getInterMergeCandidates TComDataCU.cpp:2761-3204 with
//   the micro-image candidates getMILeftCand / getMIAboveCand / getMIAboveLeftCand :2620-2748, fillMvpCand :3297-3478 and the neighbour access getPULeft ... getPUBelowLeft
//   (host/hop_spine.cpp restates the same lists for the encoder: merge_candidates, fill_mvp_cand, mi_cand, nb_*; here they read a plain hop_cu_part array).
//
// The configuration is the writer's.  Termination and bounds: every loop is bounded by the picture's geometry or a constant, unary and Exp-Golomb prefixes have a hard
// cap, every value that becomes an index or a stored field is bounded first, no byte at or past data + size is read (the coder sees zeros there), and a violation sets a
// flag that stops the substream at the end of the current CTU's walk; nothing is ever stored outside the CTU's own 256 parts, 6144 levels and 3 SAO records.

#define PA_ERR_END 1u      // a byte at or past the end of the substream was asked for
#define PA_ERR_RANGE 2u    // a value out of range (a prefix beyond its cap, a vector component beyond 16 bits, a last position outside its block)
#define PA_ERR_TERM 4u     // a terminating bin with the wrong value, the stop pattern of TDecBinCABAC::finish missing, or a consumed length other than the substream's

// the decoder: TDecBinCABAC's registers, the byte cursor, the context models and parseCoeffNxN's pos / absCoeff of the current coefficient group
struct ParDec {
  uint32_t range, value; int32_t bits_needed;
  const uint8_t* data; uint32_t pos, size;   // bytes come from data[pos] while pos < size; pos runs on past it
  uint32_t flags; int32_t err_ctu;           // PA_ERR_*; the CTU (raster address) that raised the first
  uint32_t abs_coeff[16]; uint16_t cg_pos[16];
  uint8_t st[EN_STATES];
};
// one picture as the walk sees it: e is the writer's view of the same arrays (en_part, en_mpm read it), parts / levels / sao the outputs
struct ParPic {
  EntPic e;
  int32_t wpp, sao_shift, mi_size, mi_merge;  // sao_shift: bit depth - min(bit depth, 10) (invertQuantOffsets); mi_merge: the micro-image candidates (the HOP configuration)
  hop_cu_part* parts; int32_t* levels; hop_sao_param* sao;   // levels may be NULL: parsed and dropped
};

ENT_FN void pa_flag(ParDec& k, uint32_t f) { k.flags |= f; }
ENT_FN uint32_t pa_byte(ParDec& k) {                                       // TComInputBitstream::readByte with the hard end
  uint32_t b = 0;
  if (k.pos < k.size) b = k.data[k.pos]; else pa_flag(k, PA_ERR_END);
  if (k.pos != 0xFFFFFFFFu) k.pos++;
  return b;
}
ENT_FN void pa_start(ParDec& k) {                                          // TDecBinCABAC::start (:65-72)
  k.range = 510; k.bits_needed = -8;
  k.value = pa_byte(k) << 8; k.value |= pa_byte(k);
}
ENT_FN uint32_t pa_bin(ParDec& k, int idx) {                               // decodeBin (:100-143)
  const uint32_t s = k.st[idx];
  const uint32_t lps = en_lps[s >> 1][(k.range >> 6) & 3];
  k.range -= lps;
  const uint32_t scaled = k.range << 7;
  if (k.value < scaled) {
    k.st[idx] = en_next_mps[s];
    if (scaled >= (256u << 7)) return s & 1u;
    k.range = scaled >> 6; k.value += k.value;
    if (++k.bits_needed == 0) { k.bits_needed = -8; k.value += pa_byte(k); }
    return s & 1u;
  }
  const int nb = en_renorm[lps >> 3];
  k.value = (k.value - scaled) << nb; k.range = lps << nb;
  k.st[idx] = en_next_lps[s];
  k.bits_needed += nb;
  if (k.bits_needed >= 0) { k.value += pa_byte(k) << k.bits_needed; k.bits_needed -= 8; }
  return 1u - (s & 1u);
}
ENT_FN uint32_t pa_ep(ParDec& k) {                                         // decodeBinEP (:146-163)
  k.value += k.value;
  if (++k.bits_needed >= 0) { k.bits_needed = -8; k.value += pa_byte(k); }
  const uint32_t scaled = k.range << 7;
  if (k.value >= scaled) { k.value -= scaled; return 1; }
  return 0;
}
ENT_FN uint32_t pa_eps(ParDec& k, int n) {                                 // decodeBinsEP (:165-209), n <= 24
  uint32_t bins = 0;
  if (n <= 0) return 0;
  while (n > 8) {
    k.value = (k.value << 8) + (pa_byte(k) << (8 + k.bits_needed));
    uint32_t scaled = k.range << 15;
    for (int i = 0; i < 8; i++) { bins += bins; scaled >>= 1; if (k.value >= scaled) { bins++; k.value -= scaled; } }
    n -= 8;
  }
  k.bits_needed += n; k.value <<= n;
  if (k.bits_needed >= 0) { k.value += pa_byte(k) << k.bits_needed; k.bits_needed -= 8; }
  uint32_t scaled = k.range << (n + 7);
  for (int i = 0; i < n; i++) { bins += bins; scaled >>= 1; if (k.value >= scaled) { bins++; k.value -= scaled; } }
  return bins;
}
ENT_FN uint32_t pa_trm(ParDec& k) {                                        // decodeBinTrm (:212-235)
  k.range -= 2;
  const uint32_t scaled = k.range << 7;
  if (k.value >= scaled) return 1;
  if (scaled < (256u << 7)) {
    k.range = scaled >> 6; k.value += k.value;
    if (++k.bits_needed == 0) { k.bits_needed = -8; k.value += pa_byte(k); }
  }
  return 0;
}
// the end of a substream: the terminating bin 1, TDecBinCABAC::finish's stop pattern in the last byte read (:75-82), and -- readOutTrailingBits has nothing left to
// read, the decoder takes whole bytes -- a consumed length that is the substream's
ENT_FN void pa_finish_substream(ParDec& k) {
  if (!pa_trm(k)) { pa_flag(k, PA_ERR_TERM); return; }
  if (k.flags & PA_ERR_END) return;
  const uint32_t last = k.data[k.pos - 1];                                  // pos >= 2 (pa_start) and no byte was missing: pos <= size
  if (((last << (8 + k.bits_needed)) & 0xFFu) != 0x80u || k.pos != k.size) pa_flag(k, PA_ERR_TERM);
}
ENT_FN uint32_t pa_ep_exgolomb(ParDec& k, uint32_t cnt) {                  // xReadEpExGolomb; a prefix beyond what a 16-bit value needs is refused
  uint32_t sym = 0, bit = 1;
  while (bit) {
    if (cnt > 16) { pa_flag(k, PA_ERR_RANGE); return 0; }
    bit = pa_ep(k); sym += bit << cnt; cnt++;
  }
  if (--cnt) sym += pa_eps(k, (int)cnt);
  return sym;
}
ENT_FN uint32_t pa_coef_remain(ParDec& k, uint32_t rice) {                 // xReadCoefRemainExGolomb; 16-bit levels need at most 18 ones (en_code_tu), 20 is the cap
  uint32_t ones = 0;
  while (pa_ep(k)) { if (++ones > 20) { pa_flag(k, PA_ERR_RANGE); return 0; } }
  if (ones < 3) return (ones << rice) + pa_eps(k, (int)rice);
  return (((1u << (ones - 3)) + 3 - 1) << rice) + pa_eps(k, (int)(ones - 3 + rice));
}

// ---- parseCoeffNxN (:1556-1830) with parseLastSignificantXY (:1497-1554) and the transform-skip flag (:1449-1485): returns the flag; coef == NULL: parsed and dropped.
// The levels buffer holds zeros: only the non-zero levels are stored, each inside the block's 1 << 2 * log2 entries, clipped to 16 bits ----
ENT_FN int pa_parse_tu(ParDec& k, int32_t* coef, const int log2, const int chroma, const int scan_idx, const uint16_t* scans) {
  const int so = (log2 == 2) ? 0 : (log2 == 3) ? 16 : (log2 == 4) ? 80 : 336, co = (log2 == 2) ? 0 : (log2 == 3) ? 1 : (log2 == 4) ? 5 : 21;
  const uint16_t* scan = scans + scan_idx * 1360 + so; const uint16_t* scanCG = scans + 4080 + scan_idx * 85 + co;
  const int width = 1 << log2, nco = width * width;
  int ts = 0;
  if (width == 4) ts = (int)pa_bin(k, EN_TS + chroma);
  int posX, posY;
  {
    const int gMax = en_group_idx[width - 1];
    const int cb = log2 - 2;
    const int off = chroma ? 0 : (cb * 3 + ((cb + 1) >> 2)), shf = chroma ? cb : ((cb + 3) >> 2);
    const int bx = EN_LAST_X + 15 * chroma + off, by = EN_LAST_Y + 15 * chroma + off;
    for (posX = 0; posX < gMax; posX++) if (!pa_bin(k, bx + (posX >> shf))) break;
    for (posY = 0; posY < gMax; posY++) if (!pa_bin(k, by + (posY >> shf))) break;
    if (posX > 3) { const int cnt = (posX - 2) >> 1; posX = en_min_in_group[posX] + (int)pa_eps(k, cnt); }
    if (posY > 3) { const int cnt = (posY - 2) >> 1; posY = en_min_in_group[posY] + (int)pa_eps(k, cnt); }
    if (scan_idx == 2) { const int t = posX; posX = posY; posY = t; }
  }
  if (posX >= width || posY >= width) { pa_flag(k, PA_ERR_RANGE); return ts; }
  const int posLast = posX + (posY << log2);
  int scanPosLast = 0;
  while (scanPosLast < nco - 1 && scan[scanPosLast] != posLast) scanPosLast++;
  const int baseCG = EN_SIG_CG + 2 * chroma, baseSig = EN_SIG + (chroma ? 27 : 0);
  const int numBlkSide = width >> 2, lastScanSet = scanPosLast >> 4;
  unsigned long long cgFlag = 0;
  unsigned c1 = 1, goRice = 0;
  int scanPosSig = scanPosLast;
  for (int subSet = lastScanSet; subSet >= 0; subSet--) {
    const int subPos = subSet << 4;
    int numNonZero = 0, lastNZ = -1, firstNZ = 16;
    goRice = 0;
    if (scanPosSig == scanPosLast) { lastNZ = scanPosSig; firstNZ = scanPosSig; scanPosSig--; k.cg_pos[0] = (uint16_t)posLast; numNonZero = 1; }
    const int cgBlkPos = scanCG[subSet], cgPosY = cgBlkPos / numBlkSide, cgPosX = cgBlkPos - cgPosY * numBlkSide;
    unsigned r = 0, l = 0;
    if (cgPosX < numBlkSide - 1) r = (unsigned)((cgFlag >> (cgPosY * numBlkSide + cgPosX + 1)) & 1ull);
    if (cgPosY < numBlkSide - 1) l = (unsigned)((cgFlag >> ((cgPosY + 1) * numBlkSide + cgPosX)) & 1ull);
    if (subSet == lastScanSet || subSet == 0) cgFlag |= 1ull << cgBlkPos;
    else if (pa_bin(k, baseCG + ((r || l) ? 1 : 0))) cgFlag |= 1ull << cgBlkPos;
    if ((cgFlag >> cgBlkPos) & 1ull) {
      const int patternSigCtx = (width == 4) ? -1 : (int)(r + (l << 1));
      for (; scanPosSig >= subPos; scanPosSig--) {
        const int blkPos = scan[scanPosSig], pY = blkPos >> log2, pX = blkPos - (pY << log2);
        int sig = 1;
        if (scanPosSig > subPos || subSet == 0 || numNonZero) {
          int ctxSig;                                                    // getSigCtxInc, TComTrQuant.cpp:2038-2092
          if (pX + pY == 0) ctxSig = 0;
          else if (log2 == 2) ctxSig = en_ctx_ind_map[4 * pY + pX];
          else {
            const int offset = log2 == 3 ? (scan_idx == 0 ? 9 : 15) : (!chroma ? 21 : 12);
            const int xs = pX & 3, ys = pY & 3;
            int cnt;
            if (patternSigCtx == 0) cnt = xs + ys <= 2 ? (xs + ys == 0 ? 2 : 1) : 0;
            else if (patternSigCtx == 1) cnt = ys <= 1 ? (ys == 0 ? 2 : 1) : 0;
            else if (patternSigCtx == 2) cnt = xs <= 1 ? (xs == 0 ? 2 : 1) : 0;
            else cnt = 2;
            ctxSig = ((!chroma && ((pX >> 2) + (pY >> 2)) > 0) ? 3 : 0) + offset + cnt;
          }
          sig = (int)pa_bin(k, baseSig + ctxSig);
        }
        if (sig) {                                                       // at most 16 positions per group, the last position counted
          k.cg_pos[numNonZero & 15] = (uint16_t)blkPos; numNonZero++;
          if (lastNZ == -1) lastNZ = scanPosSig;
          firstNZ = scanPosSig;
        }
      }
    } else scanPosSig = subPos - 1;
    if (numNonZero > 16) { pa_flag(k, PA_ERR_RANGE); return ts; }           // (cannot happen: a group has 16 positions)
    if (numNonZero > 0) {
      const int signHidden = (lastNZ - firstNZ >= 4);                     // sign_data_hiding
      unsigned ctxSet = (subSet > 0 && !chroma) ? 2 : 0;
      if (c1 == 0) ctxSet++;
      c1 = 1;
      const int baseOne = EN_ONE + (chroma ? 16 : 0) + 4 * ctxSet;
      for (int i = 0; i < numNonZero; i++) k.abs_coeff[i] = 1;
      const int numC1 = numNonZero < 8 ? numNonZero : 8;
      int firstC2 = -1;
      for (int idx = 0; idx < numC1; idx++) {
        const uint32_t b = pa_bin(k, baseOne + (int)c1);
        if (b) { c1 = 0; if (firstC2 == -1) firstC2 = idx; }
        else if ((c1 < 3) && (c1 > 0)) c1++;
        k.abs_coeff[idx] = b + 1;
      }
      if (c1 == 0 && firstC2 != -1) k.abs_coeff[firstC2] = pa_bin(k, EN_ABS + (chroma ? 4 : 0) + (int)ctxSet) + 2;
      const int nSigns = signHidden ? numNonZero - 1 : numNonZero;
      uint32_t coeffSigns = pa_eps(k, nSigns);
      if (nSigns) coeffSigns <<= 32 - nSigns;
      int firstCoeff2 = 1;
      if (c1 == 0 || numNonZero > 8) {
        for (int idx = 0; idx < numNonZero; idx++) {
          const uint32_t baseLevel = (idx < 8) ? (uint32_t)(2 + firstCoeff2) : 1u;
          if (k.abs_coeff[idx] == baseLevel) {
            k.abs_coeff[idx] = pa_coef_remain(k, goRice) + baseLevel;
            if (k.abs_coeff[idx] > 3u * (1u << goRice)) goRice = goRice + 1 < 4 ? goRice + 1 : 4;
          }
          if (k.abs_coeff[idx] >= 2) firstCoeff2 = 0;
        }
      }
      uint32_t absSum = 0;
      for (int idx = 0; idx < numNonZero; idx++) {
        const uint32_t a = k.abs_coeff[idx];
        absSum += a;
        int neg;
        if (idx == numNonZero - 1 && signHidden) neg = (int)(absSum & 1u);
        else { neg = (int)(coeffSigns >> 31); coeffSigns <<= 1; }
        const int32_t v = neg ? (a > 32768u ? -32768 : -(int32_t)a) : (a > 32767u ? 32767 : (int32_t)a);   // TCoeff in 16 bits
        const int at = k.cg_pos[idx];
        if (coef && at < nco) coef[at] = v;
      }
    }
  }
  return ts;
}

// ---- neighbours: TComDataCU::getPULeft / getPUAbove / getPUAboveLeft / getPUAboveRight / getPUBelowLeft for the unit at luma sample (x, y), by raster order of the CTUs
// and z-order inside one (host/hop_spine.cpp nb_*): the unit, or NULL ----
ENT_FN const hop_cu_part* pa_nb_left(const ParPic& g, int x, int y) { return x > 0 ? en_part(g.e, x - 4, y) : 0; }
ENT_FN const hop_cu_part* pa_nb_above(const ParPic& g, int x, int y) { return y > 0 ? en_part(g.e, x, y - 4) : 0; }
ENT_FN const hop_cu_part* pa_nb_above_left(const ParPic& g, int x, int y) { return (x > 0 && y > 0) ? en_part(g.e, x - 4, y - 4) : 0; }
ENT_FN const hop_cu_part* pa_nb_above_right(const ParPic& g, int x, int y) {
  if (x + 4 >= g.e.pic_w) return 0;
  const int xu = (x & 63) >> 2, yu = (y & 63) >> 2;
  bool ok;
  if (xu + 1 < 16) ok = yu ? en_zidx(xu, yu) > en_zidx(xu + 1, yu - 1) : y > 0;
  else ok = yu ? false : y > 0;
  return ok ? en_part(g.e, x + 4, y - 4) : 0;
}
ENT_FN const hop_cu_part* pa_nb_below_left(const ParPic& g, int x, int y) {
  if (y + 4 >= g.e.pic_h) return 0;
  const int xu = (x & 63) >> 2, yu = (y & 63) >> 2;
  bool ok;
  if (yu + 1 < 16) ok = xu ? en_zidx(xu, yu) > en_zidx(xu - 1, yu + 1) : x > 0;
  else ok = false;
  return ok ? en_part(g.e, x - 4, y + 4) : 0;
}
// TComDataCU::getPartIndexAndSize (TComDataCU.cpp:2210-2249) in samples
ENT_FN void pa_pu_rect(int ps, int S, int pu, int& ox, int& oy, int& w, int& h) {
  ox = oy = 0; w = h = S;
  switch (ps) {
    case 1: h = S >> 1; oy = pu ? S >> 1 : 0; break;
    case 2: w = S >> 1; ox = pu ? S >> 1 : 0; break;
    case 4: h = pu ? (S >> 2) + (S >> 1) : S >> 2; oy = pu ? S >> 2 : 0; break;
    case 5: h = pu ? S >> 2 : (S >> 2) + (S >> 1); oy = pu ? (S >> 2) + (S >> 1) : 0; break;
    case 6: w = pu ? (S >> 2) + (S >> 1) : S >> 2; ox = pu ? S >> 2 : 0; break;
    case 7: w = pu ? S >> 2 : (S >> 2) + (S >> 1); ox = pu ? (S >> 2) + (S >> 1) : 0; break;
    default: break;
  }
}
// getMILeftCand / getMIAboveCand / getMIAboveLeftCand (:2620-2748): which = 0 left, 1 above, 2 above-left; (ux, uy) = the unit whose z-index the reference hands over --
// also as the "partition index" of getPartPosition, so every PU but one at the CTU's origin reads the second PU's size (host/hop_spine.cpp mi_cand)
ENT_FN bool pa_mi_cand(const ParPic& g, int ps, int cx, int cy, int S, int which, int ux, int uy, int16_t mv[2]) {
  if (which != 1 && (ux & 63) == 0) return false;
  if (which == 1 && (uy & 63) == 0) return false;
  const int first = en_zidx((ux & 63) >> 2, (uy & 63) >> 2) == 0;
  int w = S, h = S;
  switch (ps) {                                                             // getPartPosition (:3229-3288): the size only
    case 1: h = S >> 1; break;
    case 2: w = S >> 1; break;
    case 3: w = h = S >> 1; break;
    case 4: h = first ? S >> 2 : (S >> 2) + (S >> 1); break;
    case 5: h = first ? (S >> 2) + (S >> 1) : S >> 2; break;
    case 6: w = first ? S >> 2 : (S >> 2) + (S >> 1); break;
    case 7: w = first ? (S >> 2) + (S >> 1) : S >> 2; break;
    default: break;
  }
  const int mi = g.mi_size;
  const int xs = which == 1 ? 0 : -((w + mi - 1) / mi), ys = which == 0 ? 0 : -((h + mi - 1) / mi);   // -ceil(w / mi), -ceil(h / mi)
  const int16_t mh = (int16_t)((int16_t)(xs * mi) * 4), mvv = (int16_t)((int16_t)(ys * mi) * 4);                     // (<< 2 of the reference, on a negative value)
  const int hmax = (g.e.pic_w + 8 - cx - 1) << 2, hmin = (-64 - 8 - cx + 1) * 4, vmax = (g.e.pic_h + 8 - cy - 1) << 2, vmin = (-64 - 8 - cy + 1) * 4;   // isMvInsidePic (:2598-2610)
  if (!(mh >= hmin && mh <= hmax && mvv >= vmin && mvv <= vmax)) return false;
  mv[0] = mh; mv[1] = mvv;
  return true;
}
// TComDataCU::fillMvpCand (:3297-3478), one list with the SS picture: the two candidates of PU pu of the CU (cx, cy, S, part size ps)
ENT_FN void pa_fill_mvp(const ParPic& g, int ps, int cx, int cy, int S, int pu, int16_t cand[2][2]) {
  int ox, oy, w, h; pa_pu_rect(ps, S, pu, ox, oy, w, h);
  const int ltx = cx + ox, lty = cy + oy, rtx = ltx + w - 4, rty = lty, lbx = ltx, lby = lty + h - 4;
  int16_t c[3][2]; int n = 0;
#define PA_ADD(nb) ((nb) && (nb)->ref_idx >= 0 ? ((n < 3 ? (c[n][0] = (nb)->mv[0], c[n][1] = (nb)->mv[1], 0) : 0), n++, true) : false)   /* xAddMVPCand / xAddMVPCandOrder with one SS reference */
  const hop_cu_part* bl = pa_nb_below_left(g, lbx, lby); const hop_cu_part* l = pa_nb_left(g, lbx, lby);
  bool smvp = bl && bl->pred_mode != 1;
  if (!smvp) smvp = l && l->pred_mode != 1;
  bool added = PA_ADD(bl);
  if (!added) added = PA_ADD(l);
  if (!added) { added = PA_ADD(bl); if (!added) PA_ADD(l); }
  const hop_cu_part* ar = pa_nb_above_right(g, rtx, rty); const hop_cu_part* a = pa_nb_above(g, rtx, rty); const hop_cu_part* al = pa_nb_above_left(g, ltx, lty);
  added = PA_ADD(ar);
  if (!added) added = PA_ADD(a);
  if (!added) PA_ADD(al);
  if (!smvp) {
    added = PA_ADD(ar);
    if (!added) added = PA_ADD(a);
    if (!added) PA_ADD(al);
  }
#undef PA_ADD
  if (n == 2 && c[0][0] == c[1][0] && c[0][1] == c[1][1]) n = 1;
  if (n > 2) n = 2;                                                         // AMVP_MAX_NUM_CANDS
  if (g.mi_merge) {
    if (n < 2) {
      int16_t mv[2];
      bool ok = pa_mi_cand(g, ps, cx, cy, S, 0, lbx, lby, mv);
      if (!ok) ok = pa_mi_cand(g, ps, cx, cy, S, 1, rtx, rty, mv);
      if (!ok) ok = pa_mi_cand(g, ps, cx, cy, S, 2, ltx, lty, mv);
      if (ok) { c[n][0] = mv[0]; c[n][1] = mv[1]; n++; }
    }
    if (n == 2 && c[0][0] == c[1][0] && c[0][1] == c[1][1]) n = 1;
  }
  while (n < 2) { c[n][0] = 0; c[n][1] = 0; n++; }
  for (int i = 0; i < 2; i++) { cand[i][0] = c[i][0]; cand[i][1] = c[i][1]; }
}
// TComDataCU::getInterMergeCandidates (:2761-3204), P-like slice, no temporal candidate, five candidates: the one with index `want` (0..4)
ENT_FN void pa_merge_cand(const ParPic& g, int ps, int cx, int cy, int S, int pu, int want, int16_t mv[2], int8_t& ref, uint8_t& dir) {
  int ox, oy, w, h; pa_pu_rect(ps, S, pu, ox, oy, w, h);
  const int ltx = cx + ox, lty = cy + oy, rtx = ltx + w - 4, rty = lty, lbx = ltx, lby = lty + h - 4;
  int16_t f[5][2]; int8_t fr[5]; uint8_t fd[5];
  for (int i = 0; i < 5; i++) { f[i][0] = f[i][1] = 0; fr[i] = -1; fd[i] = 0; }
  int cnt = 0;
#define PA_SAME(a, b) ((a)->inter_dir == (b)->inter_dir && (!((a)->inter_dir & 1) || ((a)->mv[0] == (b)->mv[0] && (a)->mv[1] == (b)->mv[1] && (a)->ref_idx == (b)->ref_idx)))
#define PA_TAKE(nb) do { fd[cnt] = (nb)->inter_dir; f[cnt][0] = (nb)->mv[0]; f[cnt][1] = (nb)->mv[1]; fr[cnt] = (nb)->ref_idx; cnt++; } while (0)
  do {                                                                      // (isDiffMER is always true at parallel merge level 2)
    const hop_cu_part* A1 = pa_nb_left(g, lbx, lby);
    const bool okA1 = A1 && !(pu == 1 && (ps == 2 || ps == 6 || ps == 7)) && A1->pred_mode != 1;
    if (okA1) PA_TAKE(A1);
    const hop_cu_part* B1 = pa_nb_above(g, rtx, rty);
    const bool okB1 = B1 && !(pu == 1 && (ps == 1 || ps == 4 || ps == 5)) && B1->pred_mode != 1;
    if (okB1 && (!okA1 || !PA_SAME(A1, B1))) PA_TAKE(B1);
    const hop_cu_part* B0 = pa_nb_above_right(g, rtx, rty);
    const bool okB0 = B0 && B0->pred_mode != 1;
    if (okB0 && (!okB1 || !PA_SAME(B1, B0))) PA_TAKE(B0);
    const hop_cu_part* A0 = pa_nb_below_left(g, lbx, lby);
    const bool okA0 = A0 && A0->pred_mode != 1;
    if (okA0 && (!okA1 || !PA_SAME(A1, A0))) PA_TAKE(A0);
    if (cnt < 4) {
      const hop_cu_part* B2 = pa_nb_above_left(g, ltx, lty);
      const bool okB2 = B2 && B2->pred_mode != 1;
      if (okB2 && (!okA1 || !PA_SAME(A1, B2)) && (!okB1 || !PA_SAME(B1, B2))) PA_TAKE(B2);
    }
    if (cnt == 5) break;                                                    // (four spatial candidates at most: never)
    if (g.mi_merge) {                                                       // :2942-3035, all three from the PU's first unit
      int16_t m[2];
      for (int which = 0; which < 3 && cnt < 4; which++)
        if (pa_mi_cand(g, ps, cx, cy, S, which, ltx, lty, m)) { fd[cnt] = 1; f[cnt][0] = m[0]; f[cnt][1] = m[1]; fr[cnt] = 0; cnt++; }
    }
    while (cnt < 5) { fd[cnt] = 1; f[cnt][0] = f[cnt][1] = 0; fr[cnt] = 0; cnt++; }   // zero candidates (:3177-3201)
  } while (0);
#undef PA_SAME
#undef PA_TAKE
  mv[0] = f[want][0]; mv[1] = f[want][1]; ref = fr[want]; dir = fd[want];
}

ENT_FN int pa_merge_index(ParDec& k) {                                      // parseMergeIndex, MaxNumMergeCand 5: 0..4
  int idx = 0;
  for (; idx < 4; idx++) { const uint32_t sym = idx == 0 ? pa_bin(k, EN_MERGE_IDX) : pa_ep(k); if (!sym) break; }
  return idx;
}
ENT_FN void pa_vec(ParDec& k, int base, int16_t* v, int ncomp) {            // parseMvd (2 components) / parseGT (corners 0..2: 6 components), each within int16_t
  uint32_t a[6];
  for (int i = 0; i < ncomp; i++) a[i] = pa_bin(k, base);
  for (int i = 0; i < ncomp; i++) if (a[i]) a[i] += pa_bin(k, base + 1);
  for (int i = 0; i < ncomp; i++) {
    v[i] = 0;
    if (!a[i]) continue;
    if (a[i] == 2) a[i] += pa_ep_exgolomb(k, 1);
    const uint32_t neg = pa_ep(k);
    if (a[i] > 32767u) { pa_flag(k, PA_ERR_RANGE); a[i] = 32767u; }
    v[i] = (int16_t)(neg ? -(int32_t)a[i] : (int32_t)a[i]);
  }
}
// a unit as TComDataCU::initCU leaves it, in the encoder's terms (host/hop_spine.cpp part_init): what every field the stream does not carry keeps
ENT_FN void pa_unit_init(hop_cu_part& u, int depth) {
  u.depth = (uint8_t)depth; u.pred_mode = 15; u.part_size = 15; u.skip = 0; u.merge_flag = 0; u.merge_idx = 0; u.gt_flag = 0; u.inter_dir = 0;
  u.ref_idx = -1; u.mvp_idx = -1; u.mvp_num = -1; u.luma_dir = 1; u.chroma_dir = 0; u.tr_idx = 0;
  for (int i = 0; i < 3; i++) { u.cbf[i] = 0; u.tskip[i] = 0; }
  u.mv[0] = u.mv[1] = 0; u.mvd[0] = u.mvd[1] = 0;
  for (int i = 0; i < 8; i++) u.gt[i] = 0;
}

// one CU: xDecodeCU from the skip flag on (TDecCu.cpp:290-370)
ENT_FN void pa_parse_cu(ParDec& k, const ParPic& g, const int addr, const int z, const int x, const int y, const int d) {
  hop_cu_part* P = g.parts + (size_t)addr * 256 + z;                        // the CU's units: z + parts <= 256
  int32_t* L = g.levels ? g.levels + (size_t)addr * 6144 : 0;
  const int log2_cu = 6 - d, S = 1 << log2_cu, parts = 256 >> (2 * d);
  for (int q = 0; q < parts; q++) pa_unit_init(P[q], d);
  int skip = 0;
  if (!g.e.i_slice) {                                                       // parseSkipFlag with getCtxSkipFlag (TComDataCU.cpp:1888)
    int ctx = 0;
    if (x > 0) ctx += en_part(g.e, x - 4, y)->skip ? 1 : 0;
    if (y > 0) ctx += en_part(g.e, x, y - 4)->skip ? 1 : 0;
    skip = (int)pa_bin(k, EN_SKIP + ctx);
  }
  if (skip) {
    const int idx = pa_merge_index(k);
    for (int q = 0; q < parts; q++) { P[q].pred_mode = 0; P[q].part_size = 0; P[q].skip = 1; P[q].merge_flag = 1; P[q].merge_idx = (uint8_t)idx; }
    int16_t mv[2]; int8_t ref; uint8_t dir;
    pa_merge_cand(g, 0, x, y, S, 0, idx, mv, ref, dir);
    for (int q = 0; q < parts; q++) { P[q].mv[0] = mv[0]; P[q].mv[1] = mv[1]; P[q].ref_idx = ref; P[q].inter_dir = dir; }
    return;
  }
  const int intra = g.e.i_slice ? 1 : (int)pa_bin(k, EN_PRED);
  const int is_min_cu = d == 3, amp_acc = d < 3;
  int e = 0;
  if (intra) {                                                              // parsePartSize
    if (is_min_cu) e = pa_bin(k, EN_PART) ? 0 : 3;
  } else if (!pa_bin(k, EN_PART)) {
    if (pa_bin(k, EN_PART + 1)) {
      e = 1;
      if (amp_acc && !pa_bin(k, EN_PART + 3)) e = pa_ep(k) ? 5 : 4;
    } else {
      e = 2;                                                                // (an 8x8 CU has no SS/GT NxN: the third bin is read only where log2 of the smallest CU is above 3)
      if (amp_acc && !pa_bin(k, EN_PART + 3)) e = pa_ep(k) ? 7 : 6;
    }
  }
  const int nxn = intra && e == 3;
  for (int q = 0; q < parts; q++) { P[q].pred_mode = (uint8_t)intra; P[q].part_size = (uint8_t)e; }
  int root = 1;
  if (intra) {                                                              // parseIntraDirLumaAng for all PUs, parseIntraDirChroma
    const int npu = nxn ? 4 : 1, q4 = parts >> 2, h = S >> 1;
    uint32_t mpm[4];
    for (int j = 0; j < npu; j++) mpm[j] = pa_bin(k, EN_IPRED);
    for (int j = 0; j < npu; j++) {
      int pr[3]; en_mpm(g.e, x + ((j & 1) ? h : 0), y + ((j >> 1) ? h : 0), pr);
      int dir;
      if (mpm[j]) { int i = (int)pa_ep(k); if (i) i += (int)pa_ep(k); dir = pr[i]; }
      else {
        dir = (int)pa_eps(k, 5);
        if (pr[0] > pr[1]) { const int t = pr[0]; pr[0] = pr[1]; pr[1] = t; }
        if (pr[0] > pr[2]) { const int t = pr[0]; pr[0] = pr[2]; pr[2] = t; }
        if (pr[1] > pr[2]) { const int t = pr[1]; pr[1] = pr[2]; pr[2] = t; }
        for (int q = 0; q < 3; q++) dir += (dir >= pr[q]);
      }
      const int n = nxn ? q4 : parts;
      for (int q = 0; q < n; q++) P[j * q4 + q].luma_dir = (uint8_t)dir;     // 0..34: three candidates below 35, or 31 + 3
    }
    int cdir = 36;                                                          // DM_CHROMA_IDX
    if (pa_bin(k, EN_CPRED)) {                                              // getAllowedChromaDir (TComDataCU.cpp:1746-1764)
      int allowed[4] = { 0, 26, 10, 1 };
      for (int q = 0; q < 4; q++) if (allowed[q] == P[0].luma_dir) allowed[q] = 34;
      cdir = allowed[pa_eps(k, 2) & 3u];
    }
    for (int q = 0; q < parts; q++) P[q].chroma_dir = (uint8_t)cdir;
  } else {                                                                  // decodePUWise
    const int npu = e == 0 ? 1 : 2;
    for (int j = 0; j < npu; j++) {
      int ox, oy, w, h; pa_pu_rect(e, S, j, ox, oy, w, h);
      hop_cu_part f; pa_unit_init(f, d);
      f.merge_flag = (uint8_t)pa_bin(k, EN_MERGE_FLAG);
      if (f.merge_flag) {
        f.merge_idx = (uint8_t)pa_merge_index(k);
        pa_merge_cand(g, e, x, y, S, j, f.merge_idx, f.mv, f.ref_idx, f.inter_dir);
      } else {
        f.inter_dir = 1; f.ref_idx = 0;                                     // decodeInterDirPU / decodeRefFrmIdxPU: one list, one picture
        pa_vec(k, EN_MVD, f.mvd, 2);
        f.mvp_idx = (int8_t)pa_bin(k, EN_MVP); f.mvp_num = 2;
        f.gt_flag = (uint8_t)pa_bin(k, EN_GTF);
        if (f.gt_flag) {
          pa_vec(k, EN_GT, f.gt, 6);
          f.gt[6] = (int16_t)(f.gt[0] - f.gt[2] + f.gt[4]); f.gt[7] = (int16_t)(f.gt[1] - f.gt[3] + f.gt[5]);   // the fourth corner: GT0 - GT1 + GT2 in TComMv's Short
        }
        int16_t cand[2][2]; pa_fill_mvp(g, e, x, y, S, j, cand);
        f.mv[0] = (int16_t)(cand[f.mvp_idx][0] + f.mvd[0]); f.mv[1] = (int16_t)(cand[f.mvp_idx][1] + f.mvd[1]);
      }
      for (int q = 0; q < parts; q++) {                                     // the PU's units (the next PU's lists read them)
        int x4, y4; en_zpos(z + q, x4, y4);
        const int ux = 4 * x4 - (x & 63), uy = 4 * y4 - (y & 63);
        if (ux < ox || ux >= ox + w || uy < oy || uy >= oy + h) continue;
        hop_cu_part& u = P[q];
        u.merge_flag = f.merge_flag; u.merge_idx = f.merge_idx; u.gt_flag = f.gt_flag; u.inter_dir = f.inter_dir; u.ref_idx = f.ref_idx; u.mvp_idx = f.mvp_idx; u.mvp_num = f.mvp_num;
        u.mv[0] = f.mv[0]; u.mv[1] = f.mv[1]; u.mvd[0] = f.mvd[0]; u.mvd[1] = f.mvd[1];
        for (int i = 0; i < 8; i++) u.gt[i] = f.gt[i];
      }
    }
    if (!(P[0].merge_flag && e == 0)) root = (int)pa_bin(k, EN_ROOT_CBF);   // parseQtRootCbf
  }
  if (!root) return;
  // xDecodeTransform (TDecEntropy.cpp:453-646): pre-order; the chroma cbf on the way down (a node's bit replaces the units' byte, :1446), the luma cbf and the levels at
  // the leaves, the chroma of four 4x4 luma blocks after the last, and on the way up every node's bit = the OR of its four children's (:537-552)
  const int log2_max_tu = 5;
  int log2_min_in_cu;                                                       // getQuadtreeTULog2MinSizeInCU (TComDataCU.cpp:1860-1886), QuadtreeTUMaxDepthIntra / Inter 3
  if (log2_cu < 2 + 3 - 1 + nxn) log2_min_in_cu = 2;
  else { log2_min_in_cu = log2_cu - (3 - 1 + nxn); if (log2_min_in_cu > log2_max_tu) log2_min_in_cu = log2_max_tu; }
  int sp_part[5], sp_k[5]; int sp = 0, bak = 0;
  sp_part[0] = 0; sp_k[0] = -1;
  while (sp >= 0) {
    const int part = sp_part[sp], trIdx = sp, log2 = log2_cu - sp, nu = parts >> (2 * trIdx);
    if (sp_k[sp] < 0) {
      if (log2 == 2) { const int pn = parts >> (2 * (trIdx - 1)); if (part % pn == 0) bak = part; }
      int subdiv;
      if (nxn && trIdx == 0) subdiv = 1;
      else if (log2 > log2_max_tu) subdiv = 1;
      else if (log2 == 2 || log2 == log2_min_in_cu || sp >= 3) subdiv = 0;  // (sp >= 3: the stack's bound; the minimum sizes stop every tree at depth 2, an NxN CU at 1)
      else subdiv = (int)pa_bin(k, EN_TRANS_SUBDIV + 5 - log2);
      const int first = trIdx == 0;
      for (int comp = 1; comp < 3; comp++) {
        if (first || log2 > 2) {
          if (first || ((P[part].cbf[comp] >> (trIdx - 1)) & 1)) { const uint8_t b = (uint8_t)(pa_bin(k, en_cbf_ctx(comp, trIdx)) << trIdx); for (int q = 0; q < nu; q++) P[part + q].cbf[comp] = b; }
        } else { const uint8_t b = (uint8_t)(((P[part].cbf[comp] >> (trIdx - 1)) & 1) << trIdx); for (int q = 0; q < nu; q++) P[part + q].cbf[comp] = b; }
      }
      if (!subdiv) {
        uint8_t by = (uint8_t)(1u << trIdx);
        if (intra || !(trIdx == 0 && !(P[part].cbf[1] & 1) && !(P[part].cbf[2] & 1))) by = (uint8_t)(pa_bin(k, en_cbf_ctx(0, trIdx)) << trIdx);
        for (int q = 0; q < nu; q++) { P[part + q].tr_idx = (uint8_t)trIdx; P[part + q].cbf[0] = by; }
        const int cbfY = by != 0; int cbfU = (P[part].cbf[1] >> trIdx) & 1, cbfV = (P[part].cbf[2] >> trIdx) & 1;
        int cpart = -1, clog2 = log2 - 1;
        if (log2 > 2) cpart = part;
        else { const int pn = parts >> (2 * (trIdx - 1)); if (part % pn == pn - 1) { cpart = bak; clog2 = 2; cbfU = (P[bak].cbf[1] >> trIdx) & 1; cbfV = (P[bak].cbf[2] >> trIdx) & 1; } }
        if (cbfY) {
          const int ts = pa_parse_tu(k, L ? L + 16 * (z + part) : 0, log2, 0, intra ? en_intra_scan(P[part].luma_dir, log2, 0) : 0, g.e.scans);
          if (log2 == 2) P[part].tskip[0] = (uint8_t)ts;
        }
        if (cpart >= 0) {
          const int cdir = P[0].chroma_dir == 36 ? P[0].luma_dir : P[0].chroma_dir;
          const int cscan = intra ? en_intra_scan(cdir, clog2, 1) : 0;
          for (int comp = 1; comp < 3; comp++) {
            if (!(comp == 1 ? cbfU : cbfV)) continue;
            const int ts = pa_parse_tu(k, L ? L + (comp == 1 ? 4096 : 5120) + 4 * (z + cpart) : 0, clog2, 1, cscan, g.e.scans);
            if (clog2 == 2) for (int q = 0; q < 4; q++) P[cpart + q].tskip[comp] = (uint8_t)ts;   // the 8x8 node's four units (:1462-1484)
          }
        }
        sp--; continue;
      }
      sp_k[sp] = 0;
    }
    if (sp_k[sp] < 4) { const int q = nu >> 2, kk = sp_k[sp]++; sp_part[sp + 1] = part + kk * q; sp_k[sp + 1] = -1; sp++; }
    else {
      const int q = nu >> 2;
      for (int comp = 0; comp < 3; comp++) {
        uint8_t any = 0;
        for (int kk = 0; kk < 4; kk++) any |= (uint8_t)((P[part + kk * q].cbf[comp] >> (trIdx + 1)) & 1);
        for (int i = 0; i < nu; i++) P[part + i].cbf[comp] |= (uint8_t)(any << trIdx);
      }
      sp--;
    }
  }
}

// parseSAOBlkParam (:1906-2029) as decompressSlice calls it (TDecSlice.cpp:312-345).  The records are hop_sao_frame's: a component the slice has switched off, or one that
// is off, is all zeros; a merged record carries, beside mode 2 and the direction, the band position and offsets of the candidate as reconstructBlkSAOParam resolves them
// (TComSampleAdaptiveOffset.cpp:305-339) -- derived, not read
ENT_FN void pa_parse_sao(ParDec& k, const ParPic& g, const int addr) {
  hop_sao_param* blk = g.sao + (size_t)addr * 3;
  const int rx = addr % g.e.wctu, ry = addr / g.e.wctu;
  for (int comp = 0; comp < 3; comp++) { hop_sao_param& p = blk[comp]; p.mode = p.type = p.aux = p.pad = 0; for (int i = 0; i < 32; i++) p.offset[i] = 0; }
  int left = 0, above = 0;
  if (rx > 0) left = (int)pa_bin(k, EN_SAO_MERGE);
  if (ry > 0 && !left) above = (int)pa_bin(k, EN_SAO_MERGE);
  if (left || above) {
    const hop_sao_param* cand = g.sao + (size_t)(left ? addr - 1 : addr - g.e.wctu) * 3;
    for (int comp = 0; comp < 3; comp++) {
      hop_sao_param& p = blk[comp]; const hop_sao_param& c = cand[comp];
      p.mode = 2; p.type = left ? 0 : 1; p.aux = c.aux;
      for (int i = 0; i < 32; i++) p.offset[i] = c.mode == 1 ? (int8_t)(c.offset[i] * (1 << g.sao_shift)) : c.offset[i];
    }
    return;
  }
  for (int comp = 0; comp < 3; comp++) {
    if (!(comp ? g.e.sao_chroma : g.e.sao_luma)) continue;
    hop_sao_param& p = blk[comp];
    if (comp < 2) {                                                         // parseSaoTypeIdx
      if (pa_bin(k, EN_SAO_TYPE)) { p.mode = 1; p.type = pa_ep(k) ? 0 : 4; }
    } else { p.mode = blk[1].mode; p.type = blk[1].type; }
    if (p.mode != 1) continue;
    int off[4];
    for (int i = 0; i < 4; i++) {                                           // parseSaoMaxUvlc: truncated unary, bypass, at most sao_max_offset (<= 31)
      int v = 0;
      while (v < g.e.sao_max_offset && pa_ep(k)) v++;
      off[i] = v;
    }
    if (p.type == 4) {
      for (int i = 0; i < 4; i++) if (off[i] && pa_ep(k)) off[i] = -off[i];
      p.aux = (int8_t)pa_eps(k, 5);                                         // sao_band_position: 0..31
      for (int i = 0; i < 4; i++) p.offset[(p.aux + i) & 31] = (int8_t)off[i];
    } else {
      if (comp < 2) p.type = (int8_t)pa_eps(k, 2);                          // sao_eo_class: 0..3
      p.offset[0] = (int8_t)off[0]; p.offset[1] = (int8_t)off[1]; p.offset[3] = (int8_t)-off[2]; p.offset[4] = (int8_t)-off[3];
    }
  }
}

// one CTU of decompressSlice's loop: its SAO parameters, TDecCu::decodeCU (the coding quadtree with the split flags, getCtxSplitFlag TComDataCU.cpp:1832; the units
// outside the picture as the encoder leaves them), and the terminating bins: 0 unless the CTU is the picture's last (xDecodeSliceEnd), then 1 with the finish at a
// substream's end.  A substream with a flag raised parses nothing more.
ENT_FN void pa_parse_ctu(ParDec& k, const ParPic& g, const int addr) {
  if (k.flags) return;
  if (g.sao && (g.e.sao_luma || g.e.sao_chroma)) pa_parse_sao(k, g, addr);
  const int cx = (addr % g.e.wctu) * 64, cy = (addr / g.e.wctu) * 64;
  hop_cu_part* P = g.parts + (size_t)addr * 256;
  int sp_z[4], sp_k[4]; int sp = 0;
  sp_z[0] = 0; sp_k[0] = -1;
  while (sp >= 0) {
    const int z = sp_z[sp], d = sp, size = 64 >> d;
    int x4, y4; en_zpos(z, x4, y4);
    const int x = cx + 4 * x4, y = cy + 4 * y4;
    if (sp_k[sp] < 0) {
      const bool inside = x + size <= g.e.pic_w && y + size <= g.e.pic_h;
      int split = d < 3;                                                    // a CU across the picture's border is split
      if (inside && d < 3) {
        int ctx = 0;
        if (x > 0) ctx += en_part(g.e, x - 4, y)->depth > d;
        if (y > 0) ctx += en_part(g.e, x, y - 4)->depth > d;
        split = (int)pa_bin(k, EN_SPLIT + ctx);
      }
      if (!split) { pa_parse_cu(k, g, addr, z, x, y, d); sp--; continue; }
      sp_k[sp] = 0;
    }
    if (sp_k[sp] < 4) {
      const int kk = sp_k[sp]++, h = size >> 1, cz = z + kk * (256 >> (2 * (d + 1)));
      if (x + (kk & 1) * h < g.e.pic_w && y + (kk >> 1) * h < g.e.pic_h) { sp_z[sp + 1] = cz; sp_k[sp + 1] = -1; sp++; }
      else for (int q = 0; q < (256 >> (2 * (d + 1))); q++) pa_unit_init(P[cz + q], d + 1);
    } else sp--;
  }
  const int last = addr == g.e.wctu * g.e.hctu - 1;
  if (!last && pa_trm(k)) pa_flag(k, PA_ERR_TERM);
  if (!k.flags && (g.wpp ? addr % g.e.wctu == g.e.wctu - 1 : last)) pa_finish_substream(k);
  if (k.flags && k.err_ctu < 0) k.err_ctu = addr;
}
// A substream's first bytes: start, from the context models `entry`
ENT_FN void pa_begin_substream(ParDec& k, const uint8_t* entry, const uint8_t* data, uint32_t size) {
  k.data = data; k.pos = 0; k.size = size; k.flags = 0; k.err_ctu = -1;
  pa_start(k);
  for (int i = 0; i < EN_STATES; i++) k.st[i] = entry[i];
}
