// k_pred.hip -- the final (normative, decoder-shared) inter/GT predictor and the
// distortion kernels (row a12).
// Replaces TComPrediction::xPredInterLumaBlk / xPredInterChromaBlk incl. the GT branch
// (TLibCommon/TComPrediction.cpp:639-720, :1235-1347), xPredGTLuma / xPredGTChroma (:723-805, :1351-1420),
// calcParamProjective(C) (:807-859) and ProjectiveTransform (:904-1030); DCT-IF from
// TComInterpolationFilter.cpp:55-75 (taps), :92-152 (filterCopy), :170-245 (filter<>).
// The result must be Pel-exact: the decoder runs the same double arithmetic (TDecCu.cpp:487).
// One workgroup per PU and colour plane; the doubled patch lives in LDS; IEEE double, no contraction.
#include "hop_dev.h"

#include "k_pred_dev.inl"

// grid = (n jobs, 3 planes)
__global__ __launch_bounds__(256) void k_pred_inter(const hop_pred_job* __restrict__ jobs, hop_pics pic) {
  __shared__ PredShared sh;
  const hop_pred_job jb = jobs[blockIdx.x];
  pred_inter_body<true>(sh, jb, blockIdx.y, pic);
}

int hop_launch_pred(hop_ctx* c, int n, const hop_pred_job* d_jobs) {
  const int pr = hop_prof_begin(c, HOP_K_PRED, (uint64_t)n);
  hipLaunchKernelGGL(k_pred_inter, dim3(n, 3), dim3(256), 0, c->stream, d_jobs, hop_make_pics(c));
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "pred_inter launch: %s", hipGetErrorString(e));
  return HOP_OK;
}

__global__ void k_pred_jobs_from_results(int n, const int32_t* __restrict__ index, const hop_pu_job* __restrict__ jobs,
                                         const hop_pu_result* __restrict__ res, hop_pred_job* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = index ? index[i] : i;
  const hop_pu_job jb = jobs[k];
  const hop_pu_result r = res[k];
  hop_pred_job p;
  p.pu_x = jb.pu_x; p.pu_y = jb.pu_y; p.w = jb.w; p.h = jb.h; p.dst_row_off = 0;
  if (r.not_valid) { p.mv_x = 0; p.mv_y = 0; p.use_gt = 0; for (int q = 0; q < 8; q++) p.gt[q] = 0; }
  else {
    p.mv_x = (r.mv_final[0] << 2) + (r.half_final[0] << 1) + r.qter_final[0];      // TEncSearch.cpp:4654-4656
    p.mv_y = (r.mv_final[1] << 2) + (r.half_final[1] << 1) + r.qter_final[1];
    p.use_gt = 1;
    for (int q = 0; q < 8; q++) p.gt[q] = r.gt[q];
  }
  out[i] = p;
}

extern "C" int hop_pred_jobs_from_results_device(hop_ctx* c, int n, const int32_t* d_index, const hop_pu_job* d_jobs,
                                                 const hop_pu_result* d_results, hop_pred_job* d_out) {
  if (!c || n < 0 || (n && (!d_jobs || !d_results || !d_out))) return hop_set_err(c, HOP_ERR_ARG, "hop_pred_jobs_from_results_device: bad argument");
  if (n == 0) return HOP_OK;
  hipLaunchKernelGGL(k_pred_jobs_from_results, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_index, d_jobs, d_results, d_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "pred_jobs_from_results launch: %s", hipGetErrorString(e));
  return HOP_OK;
}

// ---------------------------------------------------------------------------------------------
// distortion between the original and the prediction picture (row a12):
// SAD (TComRdCost.cpp:513-1011), SSE (:1018-1360), HADs (:1641-1708).  One workgroup per job.
// ---------------------------------------------------------------------------------------------
// one job on the 256 threads of the calling workgroup; thread 0 returns the value (barriers inside)
// tile != nullptr: the prediction is read from `tile` (pitch = the block's width) instead of the prediction picture
__device__ static uint32_t distortion_body(unsigned int& acc, const hop_dist_job& jb, const hop_pics& pic, const int16_t* tile = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool chroma = jb.comp != 0;
  const int w = chroma ? jb.w >> 1 : jb.w, h = chroma ? jb.h >> 1 : jb.h, x0 = chroma ? jb.x >> 1 : jb.x, y0 = chroma ? jb.y >> 1 : jb.y;
  const int pitch = chroma ? pic.pic_w >> 1 : pic.pic_w, bd = chroma ? pic.bd_c : pic.bd_y;
  const int16_t* o = (jb.comp == 0 ? pic.org_y : jb.comp == 1 ? pic.org_cb : pic.org_cr) + (size_t)y0 * pitch + x0;
  const int ppitch = tile ? w : pitch;
  const int16_t* p = tile ? tile : (jb.comp == 0 ? pic.pred_y : jb.comp == 1 ? pic.pred_cb : pic.pred_cr) + (size_t)y0 * pitch + x0;
  if (tid == 0) acc = 0;
  __syncthreads();
  unsigned int part = 0;
  if (jb.kind == HOP_DIST_SAD || jb.kind == HOP_DIST_SSE) {
    const unsigned sshift = (unsigned)((bd - 8) << 1);
    for (int i = tid; i < w * h; i += 256) {
      int r = i / w, c = i - r * w;
      int d = (int)o[(size_t)r * pitch + c] - (int)p[(size_t)r * ppitch + c];
      part += jb.kind == HOP_DIST_SAD ? (unsigned)(d < 0 ? -d : d) : ((unsigned)(d * d) >> sshift);
    }
    part = (unsigned)hopd_wave_sum((int)part);
    if (lane == 0) atomicAdd(&acc, part);
  } else if (((w & 7) == 0) && ((h & 7) == 0)) {
    const int nblk = (w * h) >> 6, bwb = w >> 3;
    for (int blk = wave; blk < nblk; blk += 4) {
      const int px = (blk % bwb) * 8 + (lane & 7), py = (blk / bwb) * 8 + (lane >> 3);
      int d = (int)o[(size_t)py * pitch + px] - (int)p[(size_t)py * ppitch + px];
      int s = hopd_satd8x8_wave(d, lane);
      if (lane == 0) atomicAdd(&acc, (unsigned)s);
    }
  } else {
    const int nb4 = (w >> 2) * (h >> 2), bw4 = w >> 2;
    for (int b0 = wave * 4; b0 < nb4; b0 += 16) {
      const int blk = b0 + (lane >> 4);
      const bool act = blk < nb4;
      const int bb = act ? blk : 0;
      const int px = (bb % bw4) * 4 + (lane & 3), py = (bb / bw4) * 4 + ((lane >> 2) & 3);
      int d = (int)o[(size_t)py * pitch + px] - (int)p[(size_t)py * ppitch + px];
      int sb = hopd_satd4x4_quad(act ? d : 0, lane);
      int s = hopd_wave_sum((act && (lane & 15) == 0) ? sb : 0);
      if (lane == 0) atomicAdd(&acc, (unsigned)s);
    }
  }
  __syncthreads();
  return (jb.kind == HOP_DIST_SSE) ? acc : (acc >> (bd - 8));
}
__global__ __launch_bounds__(256) void k_distortion(const hop_dist_job* __restrict__ jobs, hop_pics pic, uint32_t* __restrict__ out) {
  __shared__ unsigned int acc;
  const hop_dist_job jb = jobs[blockIdx.x];
  const uint32_t v = distortion_body(acc, jb, pic);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// Sequences of candidates rated "one after the other" (TEncSearch::xMergeEstimation TLibEncoder/TEncSearch.cpp:2992-3106, xGetTemplateCost :4411-4477 with xGetInterPredictionError
// :2951-2977: every candidate of a PU is predicted into the same temporary block and its luma distortion taken): sequence s = jobs first[s] .. first[s + 1] - 1, all on the
// PU's rectangle.  The candidates do not depend on each other -- they only share the block they are predicted into --, so every candidate gets a workgroup of its own:
// grid (jobs, 3).  Plane 0: the luma prediction into an LDS tile, its distortion against the original -> out[job]; the LAST candidate of a sequence also writes its tile to
// the prediction picture.  Planes 1 / 2: the chroma prediction of the last candidate of each sequence into the picture (the other workgroups return at once) -- afterwards
// the prediction picture holds the last candidate's prediction in all planes, as after the reference's loop.
// (three workgroups per CU fit by LDS: the register allocator is held to the 168 VGPRs that lets them run, which it met by itself before the row-limited loops joined)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_pred_cost(const int32_t* __restrict__ seq_of, const int32_t* __restrict__ first, const hop_pred_job* __restrict__ jobs,
                                                   const int32_t* __restrict__ kinds, hop_pics pic, uint32_t* __restrict__ out) {
  __shared__ PredShared sh;
  __shared__ int16_t tile[64 * 64];
  __shared__ unsigned int acc;
  const int j = blockIdx.x, comp = blockIdx.y, s = seq_of[j];
  const bool last = j == first[s + 1] - 1;
  const hop_pred_job jb = jobs[j];
  if (comp) { if (last) pred_inter_body<true>(sh, jb, comp, pic); return; }
  pred_inter_body<true>(sh, jb, 0, pic, tile);
  __syncthreads();
  hop_dist_job d; d.x = jb.pu_x; d.y = jb.pu_y + jb.dst_row_off; d.w = jb.w; d.h = jb.h; d.comp = 0; d.kind = kinds[s];
  const uint32_t v = distortion_body(acc, d, pic, tile);
  if (threadIdx.x == 0) out[j] = v;
  if (last) {
    int16_t* dst = pic.pred_y + (size_t)(jb.pu_y + jb.dst_row_off) * pic.pic_w + jb.pu_x;
    for (int i = threadIdx.x; i < jb.w * jb.h; i += 256) { const int y = i / jb.w, x = i - y * jb.w; dst[(size_t)y * pic.pic_w + x] = tile[i]; }
  }
}
int hop_launch_pred_cost(hop_ctx* c, int total, const int32_t* d_seq_of, const int32_t* d_first, const hop_pred_job* d_jobs, const int32_t* d_kinds, uint32_t* d_out) {
  const int pr = hop_prof_begin(c, HOP_K_PRED, (uint64_t)total);
  hipLaunchKernelGGL(k_pred_cost, dim3(total, 3), dim3(256), 0, c->stream, d_seq_of, d_first, d_jobs, d_kinds, hop_make_pics(c), d_out);
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "pred_cost launch: %s", hipGetErrorString(e));
  return HOP_OK;
}

int hop_launch_dist(hop_ctx* c, int n, const hop_dist_job* d_jobs, uint32_t* d_out) {
  const int pr = hop_prof_begin(c, HOP_K_DIST, (uint64_t)n);
  hipLaunchKernelGGL(k_distortion, dim3(n), dim3(256), 0, c->stream, d_jobs, hop_make_pics(c), d_out);
  hop_prof_end(c, pr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "distortion launch: %s", hipGetErrorString(e));
  return HOP_OK;
}
