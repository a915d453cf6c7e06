// k_decode.hip -- hop_decode_frame: a picture reconstructed on the device from its parsed syntax.
// Replaces the reconstruction half of the reference decoder's CTU loop: TDecCu::xDecompressCU (TLibDecoder/TDecCu.cpp:383-476) with xReconIntraQT /
// xIntraRecLumaBlk / xIntraRecChromaBlk, xReconInter -> TComPrediction::motionCompensation + TComTrQuant::invRecurTransformNxN (TLibCommon/TComTrQuant.cpp:1285-1330)
// and the SS-reference commit xFindSSRef2Copy.
// k_dec_ctu: one workgroup of 256 threads per CTU walks the CTU's CUs in z-order and calls the bodies the encoder's kernels are made of -- intra_pred_body /
// intra_pred_chroma_body (k_intra_dev.inl), pred_inter_body (k_pred_dev.inl), turd_inverse_body / turd_inverse_small_body (k_turd_dev.inl), commit_plane
// (k_ssref_dev.inl).  Every launch holds the CTUs of one level of the host's schedule (host/hop_decode.cpp); the dependencies are kept by stream order alone
// (no spin-waits, no persistent kernel), so malformed input cannot hang the device.
// hop_decode_stack: the same kernel over the pictures of a stacked context (hop_ctx_set_stack) -- what the reference does by running TDecTop::decode once per view.  A
// level's launch holds that level's CTUs of every picture; a CTU addresses the planes by the rows of the stack and reasons about edges (intra availability, clipMv, the
// margins the commit extends) in the rows of its own picture.  hop_decode_frame is the one-picture case.
#include <string.h>
#include <vector>
#include "hop_dev.h"
#include "k_intra_dev.inl"
#include "k_turd_dev.inl"
#include "k_pred_dev.inl"
#include "k_ssref_dev.inl"

extern "C" int hop_dec_plan_stack(int pic_w, int sub_h, int n_pic, int allow_inter, const hop_cu_part* parts, int schedule, int32_t* ctu_level, int32_t* n_levels,
                                  const char* noun, char* err, size_t errn);   // host/hop_decode.cpp

namespace {

struct DecShared {
  union { IntraShared in; PredShared pr; TurdFwdShared tf; TurdSmallShared ts; } u;
  hop_intra_job ij;
  hop_tu_rd_job tj;
  hop_pred_job pj;
  int64_t coef_off;
  uint32_t abs_sum, sse;
};

__device__ inline int dec_zidx(int x4, int y4) {           // g_auiRasterToZscan of a 16x16 grid of 4x4 units
  int z = 0;
  for (int b = 0; b < 4; b++) z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1));
  return z;
}
__device__ inline int dec_zpix(int px, int py) { return dec_zidx((px & 63) >> 2, (py & 63) >> 2); }
__device__ inline void dec_zpos(int z, int& x4, int& y4) {
  x4 = y4 = 0;
  for (int b = 0; b < 4; b++) { x4 |= ((z >> (2 * b)) & 1) << b; y4 |= ((z >> (2 * b + 1)) & 1) << b; }
}
// availability of the neighbour units of a block (TComDataCU::getPUAboveRightAdi / getPUBelowLeftAdi in z-order; what the encoder's spine computes, hop_spine.cpp)
// Rows are absolute (a stack's picture k starts at row top = k * sub_pitch, a multiple of 64): "above the picture" is y == top, "below it" y >= bottom = top + sub_h.
__device__ inline bool dec_ar_avail(int x, int y, int k, int pic_w, int top) {
  if (x + 4 * k >= pic_w) return false;
  if (((x & 63) >> 2) + k < 16) return (y & 63) ? dec_zpix(x, y) > dec_zpix(x + 4 * k, y - 4) : y > top;
  return (y & 63) ? false : y > top;
}
__device__ inline bool dec_bl_avail(int x, int y, int k, int bottom) {
  if (y + 4 * k >= bottom) return false;
  if (((y & 63) >> 2) + k < 16) return (x & 63) ? dec_zpix(x, y) > dec_zpix(x - 4, y + 4 * k) : x > 0;
  return false;
}
// the intra job of a luma block at (x, y) of `size` luma samples (chroma: the same flags, per 2-sample unit), filled by the workgroup; ends with a barrier
__device__ void dec_intra_job(hop_intra_job& j, int x, int y, int size, int pic_w, int top, int bottom) {
  const int tid = threadIdx.x, u = size / 4;
  if (tid == 0) { j.x = x; j.y = y; j.strong = 1; }                  // SPS strong_intra_smoothing of both configurations
  if (tid < 4 * u + 1) {
    bool a;
    if (tid == 2 * u) a = (x & 63) ? ((y & 63) ? true : y > top) : ((y & 63) ? x > 0 : (x > 0 && y > top));
    else if (tid > 3 * u) a = dec_ar_avail(x + size - 4, y, tid - 3 * u, pic_w, top);
    else if (tid > 2 * u) a = y > top;
    else if (tid >= u) a = x > 0;
    else a = dec_bl_avail(x, y + size - 4, u - tid, bottom);
    j.flags[tid] = a ? 1 : 0;
  }
  __syncthreads();
}

struct DecArgs {
  const int32_t* order; const hop_cu_part* parts; const int32_t* levels;
  hop_pics pic;                                // org = null: the intra setup reads no original
  hop_pics pic_tu;                             // org = the prediction planes: the TU bodies' distortion side output reads valid memory and is thrown away
  int16_t* rec[3]; int16_t* ss00[3];
  int wctu;
  const int32_t* qp_scaled;                    // per picture: what setQPforQuant hands to setQpParam for Y, Cb, Cr (3 values each)
  int commit;                                  // an ISS slice commits every CU to the SS reference; an I slice has none
  int n_ctu, sub_h, sub_pitch;                 // the stack: CTUs and rows of one picture, the pictures' origins sub_pitch rows apart (0: one picture of sub_h rows)
};
struct DecPic { int top, bottom; const int32_t* qp_scaled; };   // the first row of the CTU's picture and the first row below it, in the rows of the stack; its three scaled QPs

// one TU of one plane: reconstruction = clip(prediction + inverse residual), or the prediction for cbf 0.  (x, y) in luma samples, log2 in this plane's samples
__device__ void dec_tu(DecShared& sh, const DecArgs& A, const DecPic& pp, int comp, int x, int y, int log2, bool cbf, bool tskip, bool dst, const int32_t* lv) {
  const int tid = threadIdx.x, N = 1 << log2;
  const bool chroma = comp != 0;
  const int pitch = chroma ? A.pic.pic_w >> 1 : A.pic.pic_w, x0 = chroma ? x >> 1 : x, y0 = chroma ? y >> 1 : y;
  if (!cbf) {
    const int16_t* p = (comp == 0 ? A.pic.pred_y : comp == 1 ? A.pic.pred_cb : A.pic.pred_cr) + (size_t)y0 * pitch + x0;
    int16_t* r = A.rec[comp] + (size_t)y0 * pitch + x0;
    for (int i = tid; i < N * N; i += 256) { const int rr = i >> log2, cc = i & (N - 1); r[(size_t)rr * pitch + cc] = p[(size_t)rr * pitch + cc]; }
    __syncthreads();
    return;
  }
  if (tid == 0) {
    hop_tu_rd_job j; memset(&j, 0, sizeof(j));
    j.x = x; j.y = y; j.comp = comp; j.log2_size = log2; j.qp_scaled = pp.qp_scaled[comp]; j.bit_depth = chroma ? A.pic.bd_c : A.pic.bd_y;
    j.is_intra = 1;                                                    // the bodies' reconstruction path: clip(prediction + residual) into the picture
    j.use_dst = dst ? 1 : 0; j.flags = tskip ? HOP_TU_RD_TS : 0;
    sh.tj = j; sh.coef_off = 0; sh.abs_sum = 1;
  }
  __syncthreads();
  if (log2 >= 4) turd_inverse_body(sh.u.tf, 0, &sh.tj, A.pic_tu, &sh.coef_off, lv, &sh.abs_sum, &sh.sse, A.rec[0], A.rec[1], A.rec[2]);
  else if (tid < 64) turd_inverse_small_body(sh.u.ts, 0, tid, 0, &sh.tj, 1, A.pic_tu, &sh.coef_off, lv, &sh.abs_sum, &sh.sse, A.rec[0], A.rec[1], A.rec[2]);
  __syncthreads();
}

// xReconIntraQT: the luma TUs in z-order (predicted from the reconstruction, DST for 4x4), then the chroma TUs (the 4x4 chroma of four 4x4 luma TUs with the first)
__device__ void dec_intra_cu(DecShared& sh, const DecArgs& A, DecPic pp, const hop_cu_part* P, const int32_t* LV, int z, int cx, int cy, int log2cu) {
  const int np = 1 << (2 * (log2cu - 2));
  for (int u = 0; u < np;) {
    const hop_cu_part& q = P[z + u];
    const int l2 = log2cu - q.tr_idx, tn = 1 << (2 * (l2 - 2));
    int x4, y4; dec_zpos(z + u, x4, y4);
    const int x = (cx & ~63) + 4 * x4, y = (cy & ~63) + 4 * y4, N = 1 << l2;
    dec_intra_job(sh.ij, x, y, N, A.pic.pic_w, pp.top, pp.bottom);
    if (threadIdx.x == 0) sh.ij.size = N;
    __syncthreads();
    intra_pred_body(sh.u.in, &sh.ij, q.luma_dir, A.pic, A.rec[0]);
    __syncthreads();
    dec_tu(sh, A, pp, 0, x, y, l2, (q.cbf[0] >> q.tr_idx) & 1, q.tskip[0] != 0, l2 == 2, LV + 16 * (z + u));
    u += tn;
  }
  int cm = P[z].chroma_dir;
  if (cm == 36) cm = P[z].luma_dir;                                    // DM_CHROMA_IDX: the luma direction of the first PU
  for (int u = 0; u < np;) {
    const hop_cu_part& q = P[z + u];
    const int l2 = log2cu - q.tr_idx;
    int tn = 1 << (2 * (l2 - 2)), lc = l2 - 1, bit = q.tr_idx;
    if (l2 == 2) { tn = 4; lc = 2; bit = q.tr_idx - 1; }               // chroma of the parent 8x8 node, with its first 4x4 block (TDecCu.cpp:605-610)
    int x4, y4; dec_zpos(z + u, x4, y4);
    const int x = (cx & ~63) + 4 * x4, y = (cy & ~63) + 4 * y4, Nc = 1 << lc;
    dec_intra_job(sh.ij, x, y, 2 * Nc, A.pic.pic_w, pp.top, pp.bottom);
    if (threadIdx.x == 0) sh.ij.size = Nc;
    __syncthreads();
    for (int comp = 1; comp < 3; comp++) {
      intra_pred_chroma_body(sh.u.in, &sh.ij, cm, comp, A.pic, A.rec[1], A.rec[2]);
      __syncthreads();
      dec_tu(sh, A, pp, comp, x, y, lc, (q.cbf[comp] >> bit) & 1, q.tskip[comp] != 0, false, LV + (comp == 1 ? 4096 : 5120) + 4 * (z + u));
    }
    u += tn;
  }
}

__device__ void dec_pu_rect(int ps, int S, int pu, int& ox, int& oy, int& w, int& h) {   // TComDataCU::getPartIndexAndSize
  ox = oy = 0; w = h = S;
  switch (ps) {
    case 1: h = S >> 1; oy = pu ? S >> 1 : 0; break;
    case 2: w = S >> 1; ox = pu ? S >> 1 : 0; break;
    case 3: w = h = S >> 1; ox = (pu & 1) ? S >> 1 : 0; oy = (pu >> 1) ? S >> 1 : 0; break;
    case 4: h = pu ? (S >> 2) + (S >> 1) : S >> 2; oy = pu ? S >> 2 : 0; break;
    case 5: h = pu ? S >> 2 : (S >> 2) + (S >> 1); oy = pu ? (S >> 2) + (S >> 1) : 0; break;
    case 6: w = pu ? (S >> 2) + (S >> 1) : S >> 2; ox = pu ? S >> 2 : 0; break;
    case 7: w = pu ? S >> 2 : (S >> 2) + (S >> 1); ox = pu ? (S >> 2) + (S >> 1) : 0; break;
    default: break;
  }
}

// xReconInter: every PU predicted from the SS reference, then the residual quadtree added TU by TU (a skip CU or root cbf 0: the prediction)
__device__ void dec_inter_cu(DecShared& sh, const DecArgs& A, DecPic pp, const hop_cu_part* P, const int32_t* LV, int z, int cx, int cy, int log2cu) {
  const int S = 1 << log2cu, ps = P[z].part_size, npu = ps == 0 ? 1 : ps == 3 ? 4 : 2;
  const int pic_w = A.pic.pic_w;
  for (int pu = 0; pu < npu; pu++) {
    if (threadIdx.x == 0) {
      int ox, oy, w, h; dec_pu_rect(ps, S, pu, ox, oy, w, h);
      const hop_cu_part& p = P[dec_zpix(cx + ox, cy + oy)];
      hop_pred_job j; memset(&j, 0, sizeof(j));
      j.pu_x = cx + ox; j.pu_y = cy + oy; j.w = w; j.h = h;
      const int hmax = (pic_w + 8 - cx - 1) * 4, hmin = (-64 - 8 - cx + 1) * 4;                                     // clipMv at the CU, against its own picture
      const int vmax = (pp.bottom + 8 - cy - 1) * 4, vmin = (pp.top - 64 - 8 - cy + 1) * 4;
      j.mv_x = min(hmax, max(hmin, (int)p.mv[0])); j.mv_y = min(vmax, max(vmin, (int)p.mv[1]));
      j.use_gt = (!p.merge_flag && p.gt_flag) ? 1 : 0;
      for (int k = 0; k < 8; k++) j.gt[k] = p.gt[k];
      sh.pj = j;
    }
    __syncthreads();
    const hop_pred_job j = sh.pj;
    for (int comp = 0; comp < 3; comp++) { pred_inter_body<false>(sh.u.pr, j, comp, A.pic); __syncthreads(); }
  }
  const int np = 1 << (2 * (log2cu - 2));
  for (int u = 0; u < np;) {
    const hop_cu_part& q = P[z + u];
    const int l2 = log2cu - q.tr_idx, tn = 1 << (2 * (l2 - 2));
    int x4, y4; dec_zpos(z + u, x4, y4);
    const int x = (cx & ~63) + 4 * x4, y = (cy & ~63) + 4 * y4;
    dec_tu(sh, A, pp, 0, x, y, l2, (q.cbf[0] >> q.tr_idx) & 1, q.tskip[0] != 0, false, LV + 16 * (z + u));
    if (l2 > 2 || ((z + u) & 3) == 0) {
      const int lc = l2 > 2 ? l2 - 1 : 2, bit = l2 > 2 ? q.tr_idx : q.tr_idx - 1;
      for (int comp = 1; comp < 3; comp++)
        dec_tu(sh, A, pp, comp, x, y, lc, (q.cbf[comp] >> bit) & 1, q.tskip[comp] != 0, false, LV + (comp == 1 ? 4096 : 5120) + 4 * (z + u));
    }
    u += tn;
  }
}

__global__ __launch_bounds__(256) void k_dec_ctu(DecArgs A) {
  __shared__ DecShared sh;
  const int ctu = A.order[blockIdx.x];                                 // picture * n_ctu + the CTU's raster address in its picture
  const int k = ctu / A.n_ctu, a = ctu - k * A.n_ctu;
  const DecPic pp = { k * A.sub_pitch, k * A.sub_pitch + A.sub_h, A.qp_scaled + 3 * k };   // (k is the block's: a scalar address)
  const int cx0 = (a % A.wctu) * 64, cy0 = pp.top + (a / A.wctu) * 64;  // addressing stays absolute: rows of the stack
  const hop_cu_part* P = A.parts + (size_t)ctu * 256;
  const int32_t* LV = A.levels + (size_t)ctu * 6144;
  const int pw = A.pic.pic_w, ph = A.sub_h, sp = A.sub_pitch;
  for (int z = 0; z < 256;) {
    const int mode = P[z].pred_mode;
    if (mode != 0 && mode != 1) { z++; continue; }                     // MODE_NONE: outside the picture
    const int log2cu = 6 - P[z].depth;
    int x4, y4; dec_zpos(z, x4, y4);
    const int cx = cx0 + 4 * x4, cy = cy0 + 4 * y4, S = 1 << log2cu;
    if (mode == 1) dec_intra_cu(sh, A, pp, P, LV, z, cx, cy, log2cu);
    else dec_inter_cu(sh, A, pp, P, LV, z, cx, cy, log2cu);
    z += 1 << (2 * (log2cu - 2));                                      // the units of the CU
    if (!A.commit) { __syncthreads(); continue; }
    // xFindSSRef2Copy: the CU into the SS reference, its halo re-extended
    commit_plane<false>(A.ss00[0], A.pic.stride_y, pw, ph, sp, HOP_MARGIN_Y, cx, cy, S, A.rec[0], pw);
    __syncthreads();
    commit_plane<false>(A.ss00[1], A.pic.stride_c, pw >> 1, ph >> 1, sp >> 1, HOP_MARGIN_C, cx >> 1, cy >> 1, S >> 1, A.rec[1], pw >> 1);
    __syncthreads();
    commit_plane<false>(A.ss00[2], A.pic.stride_c, pw >> 1, ph >> 1, sp >> 1, HOP_MARGIN_C, cx >> 1, cy >> 1, S >> 1, A.rec[2], pw >> 1);
    __syncthreads();
  }
}

}  // namespace

static int dec_pictures(const hop_ctx* c, int* ph) {
  *ph = c->sub_pitch ? c->sub_h : c->pic_h;
  return c->sub_pitch ? (c->pic_h - c->sub_h) / c->sub_pitch + 1 : 1;
}

// internal: what hop_decode_frame, hop_decode_stack and hop_access_units_decode (csrc/k_stream.hip) share -- the checks, the plan of every picture of the context
// (from the host parts; nothing is enqueued before it stands), the reset of the SS reference and one launch per level, picture k's CTUs at [k * n_ctu, (k + 1) * n_ctu).
// d_parts == NULL: parts and `levels` (host) are uploaded into the scratch area.  Otherwise both are on the device already -- d_parts, d_levels, and d_order with room
// for one int32 per CTU of the stack and three per picture (the scaled QPs go behind the order), in memory the caller keeps in place until this returns -- and `levels`
// is not read.  pic_qp (host, one per picture of the context) or NULL: p->qp for all pictures.  Synchronous.
extern "C" __attribute__((visibility("hidden"))) int hop_dec_device(hop_ctx* c, const char* who, const char* noun, const hop_dec_params* p, const hop_cu_part* parts, const int32_t* levels,
                                                                    const hop_cu_part* d_parts, const int32_t* d_levels, int32_t* d_order, const int32_t* pic_qp) {
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "%s: a sharded context decodes no picture", who);
  if (p->schedule != 0 && p->schedule != 1) return hop_set_err(c, HOP_ERR_ARG, "%s: schedule %d", who, p->schedule);
  if (p->plain_intra != 0 && p->plain_intra != 1) return hop_set_err(c, HOP_ERR_ARG, "%s: plain_intra %d", who, p->plain_intra);
  if (!p->plain_intra && (c->bd_y != 8 || c->bd_c != 8)) return hop_set_err(c, HOP_ERR_ARG, "%s: the HOP configuration is 8 bit, the context is %d bit", who, c->bd_y);
  const int off_y = 6 * (c->bd_y - 8), off_c = 6 * (c->bd_c - 8);
  if (p->qp < -off_y || p->qp > 51 || p->cb_qp_offset < -12 || p->cb_qp_offset > 12 || p->cr_qp_offset < -12 || p->cr_qp_offset > 12)
    return hop_set_err(c, HOP_ERR_ARG, "%s: qp %d / offsets %d %d out of range", who, p->qp, p->cb_qp_offset, p->cr_qp_offset);
  c->levels_valid = false;                                              // the picture is no longer the one hop_encode_frame's resident levels belong to
  int ph; const int n_pic = dec_pictures(c, &ph);
  const int wctu = (c->pic_w + 63) / 64, hctu = (ph + 63) / 64, n_ctu = wctu * hctu, n = n_ctu * n_pic;
  std::vector<int32_t> level(n);
  int32_t n_levels = 0;
  char err[256] = { 0 };
  if (hop_dec_plan_stack(c->pic_w, ph, n_pic, !p->plain_intra, parts, p->schedule, level.data(), &n_levels, noun, err, sizeof(err)) != HOP_OK)
    return hop_set_err(c, HOP_ERR_ARG, "%s", err);
  // the CTUs of all pictures level by level (counting sort; inside a level picture after picture, raster order inside a picture)
  std::vector<int32_t> first(n_levels + 1, 0), order(n);
  for (int a = 0; a < n; a++) first[level[a] + 1]++;
  for (int l = 0; l < n_levels; l++) first[l + 1] += first[l];
  { std::vector<int32_t> at(first.begin(), first.end() - 1); for (int a = 0; a < n; a++) order[at[level[a]]++] = a; }
  // TComTrQuant::setQPforQuant (TComTrQuant.cpp:192-214), as host/hop_spine.cpp's finish_config
  static const uint8_t chroma_scale[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                            29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };
  DecArgs A;
  std::vector<int32_t> qs(3 * (size_t)n_pic);
  for (int i = 0; i < n_pic; i++) {
    const int qp = pic_qp ? pic_qp[i] : p->qp;
    if (qp < -off_y || qp > 51) return hop_set_err(c, HOP_ERR_ARG, "%s: %s %d: qp %d out of range", who, noun, i, qp);
    qs[3 * i] = qp + off_y;
    for (int k = 1; k < 3; k++) {
      const int o = k == 1 ? p->cb_qp_offset : p->cr_qp_offset;
      const int q = std::min(57, std::max(-off_c, qp + o));
      qs[3 * i + k] = q < 0 ? q + off_c : chroma_scale[q] + off_c;
    }
  }
  hipError_t e = hipSetDevice(c->device);
  if (!d_parts) {                                                       // parts and levels from the host: uploaded once, the order behind them
    const size_t b_parts = sizeof(hop_cu_part) * 256 * (size_t)n, b_levels = sizeof(int32_t) * 6144 * (size_t)n;
    const size_t o_levels = (b_parts + 255) & ~(size_t)255, o_order = (o_levels + b_levels + 255) & ~(size_t)255, total = o_order + sizeof(int32_t) * ((size_t)n + 3 * (size_t)n_pic);
    void* buf; const int r = hop_scratch(c, total, &buf); if (r) return r;
    char* b = (char*)buf;
    if (e == hipSuccess) e = hipMemcpyAsync(b, parts, b_parts, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b + o_levels, levels, b_levels, hipMemcpyHostToDevice, c->stream);
    d_parts = (const hop_cu_part*)b; d_levels = (const int32_t*)(b + o_levels); d_order = (int32_t*)(b + o_order);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_order + n, qs.data(), sizeof(int32_t) * qs.size(), hipMemcpyHostToDevice, c->stream);
  A.qp_scaled = d_order + n;
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "%s: upload: %s", who, hipGetErrorString(e));
  if (!p->plain_intra) { const int r = hop_launch_ssref_reset(c); if (r) return r; }
  A.parts = d_parts; A.levels = d_levels;
  A.pic = hop_make_pics(c); A.pic.org_y = A.pic.org_cb = A.pic.org_cr = nullptr;      // (hop_ctx_set_row_limit is an encoder's: k_dec_ctu instantiates pred_inter_body<false>, which has no limited reads at all)
  A.pic_tu = A.pic; A.pic_tu.org_y = A.pic.pred_y; A.pic_tu.org_cb = A.pic.pred_cb; A.pic_tu.org_cr = A.pic.pred_cr;
  for (int k = 0; k < 3; k++) { A.rec[k] = c->rec[k]; A.ss00[k] = c->ss00[k]; }
  A.wctu = wctu; A.commit = !p->plain_intra;
  A.n_ctu = n_ctu; A.sub_h = ph; A.sub_pitch = c->sub_pitch;
  for (int l = 0; l < n_levels; l++) {                                  // one launch per level, ordered by the stream alone
    A.order = d_order + first[l];
    if (first[l + 1] > first[l]) hipLaunchKernelGGL(k_dec_ctu, dim3(first[l + 1] - first[l]), dim3(256), 0, c->stream, A);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  return HOP_OK;
}

extern "C" int hop_decode_frame(hop_ctx* c, const hop_dec_params* p, const hop_cu_part* parts, const int32_t* levels) {
  if (!c || !p || !parts || !levels) return hop_set_err(c, HOP_ERR_ARG, "hop_decode_frame: bad argument");
  if (c->sub_pitch || c->sub_h) return hop_set_err(c, HOP_ERR_ARG, "hop_decode_frame: a stacked context decodes no picture (one picture per context)");
  return hop_dec_device(c, "hop_decode_frame", "picture", p, parts, levels, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int hop_decode_stack(hop_ctx* c, const hop_dec_params* p, const hop_cu_part* parts, const int32_t* levels) {
  if (!c || !p || !parts || !levels) return hop_set_err(c, HOP_ERR_ARG, "hop_decode_stack: bad argument");
  return hop_dec_device(c, "hop_decode_stack", "picture", p, parts, levels, nullptr, nullptr, nullptr, hop_picture_qps(c));
}

// host only; defined here, not in host/hop_decode.cpp, because the reason of a refusal goes where hop_last_error(NULL) reads it
extern "C" int hop_decode_stack_schedule(int pic_w, int sub_h, int n_pictures, const hop_cu_part* parts, int schedule, int32_t* ctu_level, int32_t* n_levels) {
  char err[256] = { 0 };
  const int r = hop_dec_plan_stack(pic_w, sub_h, n_pictures, 1, parts, schedule, ctu_level, n_levels, "picture", err, sizeof(err));
  if (r) hop_set_err(nullptr, r, "%s", err);
  return r;
}
