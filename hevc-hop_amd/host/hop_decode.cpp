// hop_decode.cpp -- host side of hop_decode_frame and hop_decode_stack: the checks of the partition data and the schedule of the picture's CTUs, and the merge of the
// pictures' schedules for a stack (plain C++, no device code).
//
// The reference decoder reconstructs CTUs in raster order and the CUs of a CTU in z-order, and commits every CU to the SS reference as soon as it is decoded
// (TDecCu::xDecompressCU -> xFindSSRef2Copy, TLibDecoder/TDecCu.cpp:383-476).  Samples of CUs not yet decoded read as the sentinel -1, and predictions do read them.
// A parallel schedule must therefore hand every prediction exactly the SS-reference state raster order hands it: the CTUs are put into levels of a DAG whose edges
// all run from the raster-earlier CTU to the later one --
//   - intra neighbours: left, above-left, above and above-right CTU;
//   - footprint reads: for every SS/GT PU the CTUs its prediction reads (luma and chroma).  A raster-earlier CTU there must be decoded before (edge into the PU's
//     CTU), a raster-later one must still be the sentinel (edge out of the PU's CTU).
// A level only holds CTUs that neither read nor write each other's samples, so the launches of one level may run in any order.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/hophip.h"

namespace {
const int CTU = 64, MARGIN_Y = 80, MARGIN_C = 40, GUARD = 64;   // csrc/hop_dev.h: HOP_MARGIN_Y / HOP_MARGIN_C / HOP_GUARD_ROWS
enum { MODE_INTER = 0, MODE_INTRA = 1, MODE_NONE = 15 };
enum { SIZE_2Nx2N, SIZE_2NxN, SIZE_Nx2N, SIZE_NxN, SIZE_2NxnU, SIZE_2NxnD, SIZE_nLx2N, SIZE_nRx2N };

inline void zpos(int z, int& x4, int& y4) {
  x4 = y4 = 0;
  for (int b = 0; b < 4; b++) { x4 |= ((z >> (2 * b)) & 1) << b; y4 |= ((z >> (2 * b + 1)) & 1) << b; }
}

// TComDataCU::getPartIndexAndSize (TComDataCU.cpp:2210-2249): offset and size of PU `pu` in a CU of S samples
void pu_rect(int ps, int S, int pu, int& ox, int& oy, int& w, int& h) {
  ox = oy = 0; w = h = S;
  switch (ps) {
    case SIZE_2NxN:  h = S >> 1; oy = pu ? S >> 1 : 0; break;
    case SIZE_Nx2N:  w = S >> 1; ox = pu ? S >> 1 : 0; break;
    case SIZE_NxN:   w = h = S >> 1; ox = (pu & 1) ? S >> 1 : 0; oy = (pu >> 1) ? S >> 1 : 0; break;
    case SIZE_2NxnU: h = pu ? (S >> 2) + (S >> 1) : S >> 2; oy = pu ? S >> 2 : 0; break;
    case SIZE_2NxnD: h = pu ? S >> 2 : (S >> 2) + (S >> 1); oy = pu ? (S >> 2) + (S >> 1) : 0; break;
    case SIZE_nLx2N: w = pu ? (S >> 2) + (S >> 1) : S >> 2; ox = pu ? S >> 2 : 0; break;
    case SIZE_nRx2N: w = pu ? S >> 2 : (S >> 2) + (S >> 1); ox = pu ? (S >> 2) + (S >> 1) : 0; break;
    default: break;
  }
}
inline int num_pus(int ps) { return ps == SIZE_2Nx2N ? 1 : ps == SIZE_NxN ? 4 : 2; }

struct Rect { int x0, y0, x1, y1; };   // inclusive, in samples of one plane relative to its sample (0,0)

// The samples pred_inter_body (csrc/k_pred.hip) reads for one plane of one PU.  GT: the warp's sample positions evaluated with the kernel's own double arithmetic
// (this file is built with -ffp-contract=off, as the kernel is), plus the bilinear neighbour, mapped through the doubled patch and the interpolation taps.  A warp
// whose positions are not finite integers is bounded by the kernel's clamps instead (the whole clamped window of the patch).
Rect plane_footprint(const hop_pred_job& jb, int comp) {
  const bool chroma = comp != 0;
  const int bw = chroma ? jb.w >> 1 : jb.w, bh = chroma ? jb.h >> 1 : jb.h;
  const int bx = chroma ? jb.pu_x >> 1 : jb.pu_x, by = chroma ? jb.pu_y >> 1 : jb.pu_y;
  const int ish = chroma ? 3 : 2, fmask = chroma ? 7 : 3;
  const int ix = jb.mv_x >> ish, iy = jb.mv_y >> ish, xf = jb.mv_x & fmask, yf = jb.mv_y & fmask;
  const int lo = chroma ? 1 : 3, hi = chroma ? 2 : 4;                 // taps left / right of the sample (mc_sample<4> / <8>)
  const int tl = xf ? lo : 0, tr = xf ? hi : 0, tt = yf ? lo : 0, tb = yf ? hi : 0;
  bool any = false;
  for (int k = 0; k < 8; k++) any = any || jb.gt[k] != 0;
  Rect r;
  if (!jb.use_gt || !any) {
    r.x0 = bx + ix - tl; r.x1 = bx + ix + bw - 1 + tr; r.y0 = by + iy - tt; r.y1 = by + iy + bh - 1 + tb;
    return r;
  }
  const int nssWindow = (std::min(bh, bw) >> 1) * 2;
  int lastStepI = nssWindow >> 6; if (lastStepI == 0) lastStepI = 1;
  const int m = nssWindow / 2;
  // patch rows / columns the warp can reach after the kernel's clamps (centre = patch + (bh/2, bw/2))
  int pr0 = bh / 2 - m, pr1 = bh / 2 + m + bh - 1, pc0 = bw / 2 - m, pc1 = bw / 2 + m + bw - 1;
  double h[9];
  {
    const double Wd = (double)(2 * bw) - 1.0, Hd = (double)(2 * bh) - 1.0;
    if (!chroma) {
      const int cx0 = jb.gt[0] * lastStepI, cx1 = jb.gt[2] * lastStepI + 2 * bw - 1, cx2 = jb.gt[4] * lastStepI + 2 * bw - 1, cx3 = jb.gt[6] * lastStepI;
      const int cy0 = jb.gt[1] * lastStepI, cy1 = jb.gt[3] * lastStepI, cy2 = jb.gt[5] * lastStepI + 2 * bh - 1, cy3 = jb.gt[7] * lastStepI + 2 * bh - 1;
      const double dx1 = (double)cx1 - cx2, dx2 = (double)cx3 - cx2, dx3 = (double)cx0 - cx1 + cx2 - cx3;
      const double dy1 = (double)cy1 - cy2, dy2 = (double)cy3 - cy2, dy3 = (double)cy0 - cy1 + cy2 - cy3;
      h[2] = ((dx3 * dy2 - dx2 * dy3) / (dx1 * dy2 - dx2 * dy1)) / Wd;
      h[5] = ((dx1 * dy3 - dx3 * dy1) / (dx1 * dy2 - dx2 * dy1)) / Hd;
      h[0] = (double)(cx1 - cx0) / Wd + h[2] * cx1;
      h[3] = (double)(cx3 - cx0) / Hd + h[5] * cx3;
      h[6] = (double)cx0;
      h[1] = (double)(cy1 - cy0) / Wd + h[2] * cy1;
      h[4] = (double)(cy3 - cy0) / Hd + h[5] * cy3;
      h[7] = (double)cy0;
    } else {
      const double ls = (double)lastStepI;
      const double x0 = ((double)jb.gt[0] / 2) * ls, y0 = ((double)jb.gt[1] / 2) * ls;
      const double x1 = (((double)jb.gt[2] / 2) * ls) + 2 * bw - 1, y1 = ((double)jb.gt[3] / 2) * ls;
      const double x2 = (((double)jb.gt[4] / 2) * ls) + 2 * bw - 1, y2 = (((double)jb.gt[5] / 2) * ls) + 2 * bh - 1;
      const double x3 = ((double)jb.gt[6] / 2) * ls, y3 = (((double)jb.gt[7] / 2) * ls) + 2 * bh - 1;
      const double dx1 = x1 - x2, dx2 = x3 - x2, dx3 = x0 - x1 + x2 - x3;
      const double dy1 = y1 - y2, dy2 = y3 - y2, dy3 = y0 - y1 + y2 - y3;
      h[2] = ((dx3 * dy2 - dx2 * dy3) / (dx1 * dy2 - dx2 * dy1)) / Wd;
      h[5] = ((dx1 * dy3 - dx3 * dy1) / (dx1 * dy2 - dx2 * dy1)) / Hd;
      h[0] = (x1 - x0) / Wd + h[2] * x1;
      h[3] = (x3 - x0) / Hd + h[5] * x3;
      h[6] = x0;
      h[1] = (y1 - y0) / Wd + h[2] * y1;
      h[4] = (y3 - y0) / Hd + h[5] * y3;
      h[7] = y0;
    }
    h[8] = 1.0;
  }
  const int offX = bw - bw / 2, offY = bh - bh / 2;
  int X0 = 1 << 30, X1 = -(1 << 30), Y0 = 1 << 30, Y1 = -(1 << 30);
  bool bounded = true;
  for (int py = 0; py < bh && bounded; py++)
    for (int px = 0; px < bw; px++) {
      const int x = px + offX, y = py + offY;
      const double Fx = (h[0] * x + h[3] * y + h[6]) / (h[2] * x + h[5] * y + h[8]);
      const double Fy = (h[1] * x + h[4] * y + h[7]) / (h[2] * x + h[5] * y + h[8]);
      if (!(fabs(Fx) < 1e9) || !(fabs(Fy) < 1e9)) { bounded = false; break; }     // (int) of it is not defined: fall back to the clamps
      int Y = (int)Fy - offY, X = (int)Fx - offX;
      if (Y < -m) Y = -m;
      if (X < -m) X = -m;
      if (Y > m + bh - 1) Y = m + bh - 1;
      if (X > m + bw - 1) X = m + bw - 1;
      if (Y + 1 > m + bh - 1) Y = m + bh - 2;
      if (X + 1 > m + bw - 1) X = m + bw - 2;
      X0 = std::min(X0, X); X1 = std::max(X1, X + 1); Y0 = std::min(Y0, Y); Y1 = std::max(Y1, Y + 1);
    }
  if (bounded) { pr0 = bh / 2 + Y0; pr1 = bh / 2 + Y1; pc0 = bw / 2 + X0; pc1 = bw / 2 + X1; }
  const int ox = bx + ix - bw / 2, oy = by + iy - bh / 2;          // patch sample (0,0) in the plane
  r.x0 = ox + pc0 - tl; r.x1 = ox + pc1 + tr; r.y0 = oy + pr0 - tt; r.y1 = oy + pr1 + tb;
  return r;
}

// the CTUs whose samples a plane rectangle reads: margin samples belong to the CTU of the border sample they replicate, guard rows to none.
// false: the rectangle leaves the padded plane plus guard rows.
bool rect_ctus(const Rect& r, int pw, int ph, int margin, int ctu, int wctu, std::vector<int>& out) {
  if (r.x0 < -margin || r.x1 >= pw + margin || r.y0 < -margin - GUARD || r.y1 >= ph + margin + GUARD) return false;
  const int ya = std::max(r.y0, -margin), yb = std::min(r.y1, ph + margin - 1);
  if (ya > yb) return true;                                         // guard rows only: constant sentinel
  const int cy0 = std::min(std::max(ya, 0), ph - 1) / ctu, cy1 = std::min(std::max(yb, 0), ph - 1) / ctu;
  const int cx0 = std::min(std::max(r.x0, 0), pw - 1) / ctu, cx1 = std::min(std::max(r.x1, 0), pw - 1) / ctu;
  for (int cy = cy0; cy <= cy1; cy++) for (int cx = cx0; cx <= cx1; cx++) out.push_back(cy * wctu + cx);
  return true;
}

bool pu_footprint(int pic_w, int pic_h, const hop_pred_job& jb, std::vector<int>& out) {
  const int wctu = (pic_w + CTU - 1) / CTU;
  out.clear();
  if (!rect_ctus(plane_footprint(jb, 0), pic_w, pic_h, MARGIN_Y, CTU, wctu, out)) return false;
  if (!rect_ctus(plane_footprint(jb, 1), pic_w >> 1, pic_h >> 1, MARGIN_C, CTU >> 1, wctu, out)) return false;
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return true;
}

// TComDataCU::clipMv (TComDataCU.cpp:3492-3504) at the CU's position, and the predictor job of PU `pu` as the encoder's spine builds it
void pu_job(int pic_w, int pic_h, int cu_x, int cu_y, int S, const hop_cu_part* P, int cu_z, int pu, hop_pred_job& j) {
  int ox, oy, w, h; pu_rect(P[cu_z].part_size, S, pu, ox, oy, w, h);
  const int lx = (cu_x & 63) + ox, ly = (cu_y & 63) + oy;
  int z = 0;
  for (int b = 0; b < 4; b++) z |= (((lx >> 2 >> b) & 1) << (2 * b)) | (((ly >> 2 >> b) & 1) << (2 * b + 1));
  const hop_cu_part& p = P[z];
  memset(&j, 0, sizeof(j));
  j.pu_x = cu_x + ox; j.pu_y = cu_y + oy; j.w = w; j.h = h;
  const int hmax = (pic_w + 8 - cu_x - 1) * 4, hmin = (-CTU - 8 - cu_x + 1) * 4, vmax = (pic_h + 8 - cu_y - 1) * 4, vmin = (-CTU - 8 - cu_y + 1) * 4;
  j.mv_x = std::min(hmax, std::max(hmin, (int)p.mv[0])); j.mv_y = std::min(vmax, std::max(vmin, (int)p.mv[1]));
  j.use_gt = (!p.merge_flag && p.gt_flag) ? 1 : 0;
  for (int k = 0; k < 8; k++) j.gt[k] = p.gt[k];
}

int fail(char* err, size_t n, const char* what, int ctu, int z) {
  if (err && n) snprintf(err, n, "hop_decode: CTU %d unit %d: %s", ctu, z, what);
  return HOP_ERR_ARG;
}

// The checks of one picture's partition data, and per SS/GT PU its footprint CTUs (cb(ctu, footprint) for each).  allow_inter: SS/GT CUs may occur.
template <class F>
int walk_parts(int pic_w, int pic_h, const hop_cu_part* parts, bool allow_inter, char* err, size_t errn, F cb) {
  const int wctu = (pic_w + CTU - 1) / CTU, hctu = (pic_h + CTU - 1) / CTU;
  std::vector<int> fp;
  for (int a = 0; a < wctu * hctu; a++) {
    const hop_cu_part* P = parts + (size_t)a * 256;
    const int cx = (a % wctu) * CTU, cy = (a / wctu) * CTU;
    int z = 0;
    while (z < 256) {
      int x4, y4; zpos(z, x4, y4);
      const int ux = cx + 4 * x4, uy = cy + 4 * y4;
      const bool inside = ux < pic_w && uy < pic_h;
      const hop_cu_part& p = P[z];
      if (!inside) { if (p.pred_mode != MODE_NONE) return fail(err, errn, "a unit outside the picture is not MODE_NONE", a, z); z++; continue; }
      if (p.depth > 3) return fail(err, errn, "depth above 3", a, z);
      const int d = p.depth, S = CTU >> d, np = 256 >> (2 * d);
      if (z % np) return fail(err, errn, "CU not aligned to its depth", a, z);
      if (ux + S > pic_w || uy + S > pic_h) return fail(err, errn, "CU crosses the picture border", a, z);
      if (p.pred_mode != MODE_INTER && p.pred_mode != MODE_INTRA) return fail(err, errn, "prediction mode neither intra nor SS/GT", a, z);
      if (p.pred_mode == MODE_INTER && !allow_inter) return fail(err, errn, "SS/GT CU in a plain intra picture", a, z);
      const bool intra = p.pred_mode == MODE_INTRA;
      if (intra ? !(p.part_size == SIZE_2Nx2N || (p.part_size == SIZE_NxN && S == 8)) : !(p.part_size <= SIZE_Nx2N || (p.part_size >= SIZE_2NxnU && p.part_size <= SIZE_nRx2N && S >= 16)))
        return fail(err, errn, "part size not allowed for the CU", a, z);
      if (intra && p.chroma_dir > 34 && p.chroma_dir != 36) return fail(err, errn, "chroma direction outside 0..34 and DM", a, z);
      const int log2cu = 6 - d;
      for (int u = 0; u < np; u++) {
        const hop_cu_part& q = P[z + u];
        if (q.depth != p.depth || q.pred_mode != p.pred_mode || q.part_size != p.part_size || (intra && q.chroma_dir != p.chroma_dir))
          return fail(err, errn, "inconsistent depth, mode, part size or chroma direction inside a CU", a, z + u);
        if (intra && q.luma_dir > 34) return fail(err, errn, "luma direction outside 0..34", a, z + u);
        const int l2 = log2cu - q.tr_idx;
        if (l2 < 2 || l2 > 5 || (intra && p.part_size == SIZE_NxN && q.tr_idx < 1)) return fail(err, errn, "transform depth out of range", a, z + u);
        const int tn = 1 << (2 * (l2 - 2));                           // units of the TU
        const int t0 = u - u % tn;
        if (P[z + t0].tr_idx != q.tr_idx) return fail(err, errn, "inconsistent transform depth inside a TU", a, z + u);
        for (int c = 0; c < 3; c++) if (q.tskip[c] && ((c == 0 && l2 != 2) || (c && l2 != 3 && l2 != 2))) return fail(err, errn, "transform skip on a TU larger than 4x4", a, z + u);
      }
      if (intra && p.part_size == SIZE_2Nx2N)                                // (NxN: an 8x8 CU, one unit per PU)
        for (int u = 1; u < np; u++) if (P[z + u].luma_dir != p.luma_dir) return fail(err, errn, "inconsistent luma direction inside a PU", a, z + u);
      if (!intra) {
        for (int pu = 0; pu < num_pus(p.part_size); pu++) {
          hop_pred_job j; pu_job(pic_w, pic_h, ux, uy, S, P, z, pu, j);
          if (!pu_footprint(pic_w, pic_h, j, fp)) return fail(err, errn, "vector or GT footprint outside the padded plane and its guard rows", a, z);
          cb(a, fp);
        }
      }
      z += np;
    }
  }
  return HOP_OK;
}
}  // namespace

extern "C" {

// internal: the checks and the schedule hop_decode_frame runs (csrc/k_decode.hip), with the reason of a refusal in err
__attribute__((visibility("hidden"))) int hop_dec_plan(int pic_w, int pic_h, int allow_inter, const hop_cu_part* parts, int schedule, int32_t* ctu_level, int32_t* n_levels, char* err, size_t errn) {
  if (pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7) || !parts || !ctu_level || !n_levels || (schedule != 0 && schedule != 1)) {
    if (err && errn) snprintf(err, errn, "hop_decode: bad argument");
    return HOP_ERR_ARG;
  }
  const int wctu = (pic_w + CTU - 1) / CTU, hctu = (pic_h + CTU - 1) / CTU, n = wctu * hctu;
  std::vector<std::vector<int> > preds(n);                             // raster-earlier CTUs each CTU must come after
  const int r = walk_parts(pic_w, pic_h, parts, allow_inter != 0, err, errn, [&](int a, const std::vector<int>& fp) {
    for (size_t k = 0; k < fp.size(); k++) {
      const int b = fp[k];
      if (b < a) preds[a].push_back(b);                                // must be decoded
      else if (b > a) preds[b].push_back(a);                           // must still be the sentinel
    }
  });
  if (r) return r;
  if (schedule == 1) {
    for (int a = 0; a < n; a++) ctu_level[a] = a;
    *n_levels = n;
    return HOP_OK;
  }
  int top = 0;
  for (int a = 0; a < n; a++) {
    const int x = a % wctu, y = a / wctu;
    int lv = 0;
    if (x > 0) lv = std::max(lv, ctu_level[a - 1] + 1);                // intra neighbours
    if (y > 0) {
      lv = std::max(lv, ctu_level[a - wctu] + 1);
      if (x > 0) lv = std::max(lv, ctu_level[a - wctu - 1] + 1);
      if (x + 1 < wctu) lv = std::max(lv, ctu_level[a - wctu + 1] + 1);
    }
    for (size_t k = 0; k < preds[a].size(); k++) lv = std::max(lv, ctu_level[preds[a][k]] + 1);
    ctu_level[a] = lv;
    top = std::max(top, lv);
  }
  *n_levels = top + 1;
  return HOP_OK;
}

// internal: hop_dec_plan for the n_pic pictures of a stack (hop_decode_stack, csrc/k_decode.hip).  Every picture is planned alone, in its own coordinates; the plans
// are merged by level, so launch l holds the level-l CTUs of all pictures and *n_levels is the maximum over the pictures, not the sum (raster: CTU a of every picture in
// launch a).  parts and ctu_level: picture k's CTUs at [k * n_ctu, (k + 1) * n_ctu).  A refusal names the picture when there is more than one, by
// `noun` ("picture"; "access unit" for hop_access_units_decode).
__attribute__((visibility("hidden"))) int hop_dec_plan_stack(int pic_w, int sub_h, int n_pic, int allow_inter, const hop_cu_part* parts, int schedule, int32_t* ctu_level,
                                                               int32_t* n_levels, const char* noun, char* err, size_t errn) {
  if (n_pic < 1 || !parts || !ctu_level || !n_levels) {
    if (err && errn) snprintf(err, errn, "hop_decode: bad argument");
    return HOP_ERR_ARG;
  }
  const size_t n = (size_t)((pic_w + CTU - 1) / CTU) * ((sub_h + CTU - 1) / CTU);
  int32_t top = 0;
  for (int k = 0; k < n_pic; k++) {
    char one[200] = { 0 };
    int32_t nl = 0;
    const int r = hop_dec_plan(pic_w, sub_h, allow_inter, parts + (size_t)k * n * 256, schedule, ctu_level + (size_t)k * n, &nl, one, sizeof(one));
    if (r) {
      const char* what = strncmp(one, "hop_decode: ", 12) ? one : one + 12;
      if (err && errn) { if (n_pic > 1) snprintf(err, errn, "hop_decode: %s %d: %s", noun ? noun : "picture", k, what); else snprintf(err, errn, "%s", one); }
      return r;
    }
    top = std::max(top, nl);
  }
  *n_levels = top;
  return HOP_OK;
}

int hop_decode_schedule(int pic_w, int pic_h, const hop_cu_part* parts, int schedule, int32_t* ctu_level, int32_t* n_levels) {
  return hop_dec_plan(pic_w, pic_h, 1, parts, schedule, ctu_level, n_levels, NULL, 0);
}

int hop_decode_footprint(int pic_w, int pic_h, const hop_pred_job* pu, int32_t* ctus, int max_ctus) {
  if (pic_w <= 0 || pic_h <= 0 || !pu || max_ctus < 0 || (max_ctus && !ctus) || pu->w < 4 || pu->h < 4 || pu->w > 64 || pu->h > 64) return HOP_ERR_ARG;
  std::vector<int> fp;
  if (!pu_footprint(pic_w, pic_h, *pu, fp)) return HOP_ERR_ARG;
  for (size_t k = 0; k < fp.size() && (int)k < max_ctus; k++) ctus[k] = fp[k];
  return (int)fp.size();
}

}  // extern "C"
