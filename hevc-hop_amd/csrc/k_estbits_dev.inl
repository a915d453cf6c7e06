// k_estbits_dev.inl -- the bit-estimate table of a transform unit (TEncSbac::estBit as hop_cabac_est_bits) and the job records of the leaf step's serial stages, in two
// forms: turd_setup_body, one lane per unit (the staged k_turd_setup; the yardstick), and turd_estbits_fill / turd_records_write, a unit's table filled by all the lanes
// that serve it (the fused leaf bodies of k_leaf_fused.inl).  Plain C++ over include/hophip.h: host/hop_rdoq_host.cpp compiles both with __device__ defined away and
// tests/test_rdoq_phased_cpu.py compares them byte for byte.  Included by k_turd_dev.inl.

// one thread per TU: the bit-estimate table of its snapshot (TEncSbac::estBit as hop_cabac_est_bits) and the job records
__device__ static void turd_setup_body(const int i, const hop_tu_rd_job* __restrict__ jobs, int n, const hop_cabac_ctx* __restrict__ ctx_in, const int64_t* __restrict__ coef_off,
                             const int32_t* __restrict__ entropy_bits, hop_estbits* __restrict__ eb, hop_rdoq_job* __restrict__ rq, hop_coeff_bits_job* __restrict__ cb,
                             const uint8_t* __restrict__ state_at = nullptr /* the TU's context states, if the caller holds a copy (LDS) */) {
  if (i >= n) return;
  const hop_tu_rd_job jb = jobs[i];
  const uint8_t* s = state_at ? state_at : ctx_in[jb.ctx_index].state;
  const int width = 1 << jb.log2_size, chroma = jb.comp != 0;
  int32_t* w = (int32_t*)eb;
  for (int k = 0; k < (int)(sizeof(hop_estbits) / 4); k++) w[k] = 0;
  for (int k = 0; k < 12; k++) { eb->blockCbpBits[k][0] = entropy_bits[s[k] ^ 0]; eb->blockCbpBits[k][1] = entropy_bits[s[k] ^ 1]; }
  for (int k = 0; k < 4; k++) { eb->blockRootCbpBits[k][0] = entropy_bits[s[11 + k] ^ 0]; eb->blockRootCbpBits[k][1] = entropy_bits[s[11 + k] ^ 1]; }
  for (int k = 0; k < 2; k++) for (int b = 0; b < 2; b++) eb->significantCoeffGroupBits[k][b] = entropy_bits[s[12 + 2 * chroma + k] ^ b];
  int firstCtx = 1, numCtx = 8;
  if (width >= 16) { firstCtx = chroma ? 12 : 21; numCtx = chroma ? 3 : 6; }
  else if (width == 8) { firstCtx = 9; numCtx = chroma ? 3 : 12; }
  const int base = 16 + (chroma ? 27 : 0);
  for (int b = 0; b < 2; b++) eb->significantBits[0][b] = entropy_bits[s[base] ^ b];
  for (int k = firstCtx; k < firstCtx + numCtx; k++) for (int b = 0; b < 2; b++) eb->significantBits[k][b] = entropy_bits[s[base + k] ^ b];
  const int cbt = jb.log2_size - 2;
  const int off = chroma ? 0 : (cbt * 3 + ((cbt + 1) >> 2)), shf = chroma ? cbt : ((cbt + 3) >> 2);
  const uint8_t* px = s + 58 + 15 * chroma; const uint8_t* py = s + 88 + 15 * chroma;
  const int gmax = (width == 4) ? 3 : (width == 8) ? 5 : (width == 16) ? 7 : 9;       // g_uiGroupIdx[width - 1]
  int bitsX = 0, bitsY = 0, c;
  for (c = 0; c < gmax; c++) { const int o = off + (c >> shf); eb->lastXBits[c] = bitsX + entropy_bits[px[o] ^ 0]; bitsX += entropy_bits[px[o] ^ 1]; }
  eb->lastXBits[c] = bitsX;
  for (c = 0; c < gmax; c++) { const int o = off + (c >> shf); eb->lastYBits[c] = bitsY + entropy_bits[py[o] ^ 0]; bitsY += entropy_bits[py[o] ^ 1]; }
  eb->lastYBits[c] = bitsY;
  const int no = chroma ? 8 : 16, na = chroma ? 2 : 4, oo = 118 + (chroma ? 16 : 0), oa = 142 + (chroma ? 4 : 0);
  for (int k = 0; k < no; k++) { eb->greaterOneBits[k][0] = entropy_bits[s[oo + k] ^ 0]; eb->greaterOneBits[k][1] = entropy_bits[s[oo + k] ^ 1]; }
  for (int k = 0; k < na; k++) { eb->levelAbsBits[k][0] = entropy_bits[s[oa + k] ^ 0]; eb->levelAbsBits[k][1] = entropy_bits[s[oa + k] ^ 1]; }
  hop_rdoq_job r;
  r.log2_size = jb.log2_size; r.comp = jb.comp; r.is_intra = jb.is_intra; r.scan_idx = jb.scan_idx; r.tr_depth = jb.tr_depth; r.qp_scaled = jb.qp_scaled;
  r.bit_depth = jb.bit_depth; r.sign_hide = jb.sign_hide; r.lambda = jb.lambda_rdoq; r.coeff_offset = coef_off[i]; r.estbits_index = i; r.reserved = 0;
  rq[i] = r;
  hop_coeff_bits_job b;
  b.log2_size = jb.log2_size; b.comp = jb.comp; b.scan_idx = jb.scan_idx; b.sign_hide = jb.sign_hide; b.use_ts = jb.use_ts; b.ts_flag = (jb.flags & HOP_TU_RD_TS) ? 1 : 0; b.ctx_index = jb.ctx_index;
  b.cbf_ctx_plus1 = 1 + 4 * chroma + (chroma ? jb.tr_depth : (jb.tr_depth == 0 ? 1 : 0));           // getCtxQtCbf, TComDataCU.cpp:1848-1859
  b.coeff_offset = coef_off[i];
  cb[i] = b;
}

// The same table by the lanes that serve the unit: lane `lane` of `nlanes` writes the 32-bit words lane, lane + nlanes, ... of the 244 the table has -- every word, the
// ones turd_setup_body leaves at zero included, so the table needs no clearing pass and no word has two writers.  A [k][b] entry is one look-up that depends on nothing
// but the context states; lastXBits / lastYBits are prefix sums over at most nine entries and stay a loop, on the lane that owns their first word.  s: the unit's context
// states, entropy_bits: the 128 fractional-bit values (both in LDS in the leaf bodies).  No barrier inside: the caller places one before the table is read.
#define EB_W_SIG    4                                                 // word offsets of the members of hop_estbits
#define EB_W_LASTX  88
#define EB_W_LASTY  120
#define EB_W_ONE    152
#define EB_W_ABS    200
#define EB_W_CBP    212
#define EB_W_ROOT   236
#define EB_WORDS    244
static_assert(sizeof(hop_estbits) == EB_WORDS * 4, "hop_estbits");
__device__ static inline void turd_estbits_fill(const int lane, const int nlanes, const int log2_size, const int comp, const uint8_t* s, const int32_t* entropy_bits,
                                                hop_estbits* eb) {
  const int width = 1 << log2_size, chroma = comp != 0;
  int firstCtx = 1, numCtx = 8;
  if (width >= 16) { firstCtx = chroma ? 12 : 21; numCtx = chroma ? 3 : 6; }
  else if (width == 8) { firstCtx = 9; numCtx = chroma ? 3 : 12; }
  const int base = 16 + (chroma ? 27 : 0);
  const int cbt = log2_size - 2;
  const int off = chroma ? 0 : (cbt * 3 + ((cbt + 1) >> 2)), shf = chroma ? cbt : ((cbt + 3) >> 2);
  const int gmax = (width == 4) ? 3 : (width == 8) ? 5 : (width == 16) ? 7 : 9;       // g_uiGroupIdx[width - 1]
  const int no = chroma ? 8 : 16, na = chroma ? 2 : 4, oo = 118 + (chroma ? 16 : 0), oa = 142 + (chroma ? 4 : 0);
  int32_t* w = (int32_t*)eb;
  for (int i = lane; i < EB_WORDS; i += nlanes) {
    int at = -1;                                                      // the context whose state the word looks up; -1: the word is zero
    if (i >= EB_W_LASTX && i < EB_W_ONE) {
      const bool isY = i >= EB_W_LASTY;
      const int c0 = i - (isY ? EB_W_LASTY : EB_W_LASTX);
      if (c0 > gmax) w[i] = 0;
      else if (c0 == 0) {
        const uint8_t* p = s + (isY ? 88 : 58) + 15 * chroma;
        int32_t* out = w + (isY ? EB_W_LASTY : EB_W_LASTX);
        int bits = 0, c;
        for (c = 0; c < gmax; c++) { const int o = off + (c >> shf); out[c] = bits + entropy_bits[p[o] ^ 0]; bits += entropy_bits[p[o] ^ 1]; }
        out[c] = bits;
      }
      continue;
    }
    const int b = i & 1;
    if (i < EB_W_SIG) at = 12 + 2 * chroma + (i >> 1);
    else if (i < EB_W_LASTX) { const int k = (i - EB_W_SIG) >> 1; if (k == 0 || (k >= firstCtx && k < firstCtx + numCtx)) at = base + k; }
    else if (i < EB_W_ABS) { const int k = (i - EB_W_ONE) >> 1; if (k < no) at = oo + k; }
    else if (i < EB_W_CBP) { const int k = (i - EB_W_ABS) >> 1; if (k < na) at = oa + k; }
    else if (i < EB_W_ROOT) at = (i - EB_W_CBP) >> 1;
    else at = 11 + ((i - EB_W_ROOT) >> 1);
    w[i] = at < 0 ? 0 : entropy_bits[s[at] ^ b];
  }
}

// the records turd_setup_body writes for TU i, from the job the caller holds (off = coef_off[i])
__device__ static inline void turd_records_make(const hop_tu_rd_job& jb, const int i, const int64_t off, hop_rdoq_job& r, hop_coeff_bits_job& b) {
  const int chroma = jb.comp != 0;
  r.log2_size = jb.log2_size; r.comp = jb.comp; r.is_intra = jb.is_intra; r.scan_idx = jb.scan_idx; r.tr_depth = jb.tr_depth; r.qp_scaled = jb.qp_scaled;
  r.bit_depth = jb.bit_depth; r.sign_hide = jb.sign_hide; r.lambda = jb.lambda_rdoq; r.coeff_offset = off; r.estbits_index = i; r.reserved = 0;
  b.log2_size = jb.log2_size; b.comp = jb.comp; b.scan_idx = jb.scan_idx; b.sign_hide = jb.sign_hide; b.use_ts = jb.use_ts; b.ts_flag = (jb.flags & HOP_TU_RD_TS) ? 1 : 0; b.ctx_index = jb.ctx_index;
  b.cbf_ctx_plus1 = 1 + 4 * chroma + (chroma ? jb.tr_depth : (jb.tr_depth == 0 ? 1 : 0));           // getCtxQtCbf, TComDataCU.cpp:1848-1859
  b.coeff_offset = off;
}
