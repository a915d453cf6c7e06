// k_ssref_dev.inl -- device side of the SS-reference commit (see k_ssref.hip for what it replaces); included by k_ssref.hip and k_decode.hip
// One plane of one CU.  p00 = sample (0,0) of the padded plane; (x0,y0,s) the block in this plane's
// units; pw,ph the plane size; m its margin.  src(r,c) = value of block sample (r,c).
// Work item = one block sample; the samples on a picture edge also write their margin replicas:
//   left/right edge sample  -> m replicas on its row
//   top/bottom edge sample  -> m replicas on its column
//   corner sample           -> the m x m corner area
// A stacked context (hop_ctx_set_stack) holds independent pictures of `ph` rows whose origins lie `sub_pitch` rows apart: the block's own picture
// is the one its first row falls into, and that picture's top and bottom edges are the ones that are extended (sub_pitch 0: one picture).
template <bool PACKED>
__device__ static void commit_plane(int16_t* __restrict__ p00, int stride, int pw, int ph, int sub_pitch, int m,
                                    int x0, int y0, int s, const int16_t* __restrict__ src, int src_pitch) {
  const int n = s * s;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int r = i / s, cidx = i - r * s;
    int16_t v = PACKED ? src[i] : src[(size_t)(y0 + r) * src_pitch + x0 + cidx];
    p00[(size_t)(y0 + r) * stride + x0 + cidx] = v;
  }
  __syncthreads();   // (not needed for correctness of the replicas below, which re-read src; keeps write order tidy)
  const int x1 = x0 + s - 1, y1 = y0 + s - 1;
  const int top = sub_pitch ? (y0 / sub_pitch) * sub_pitch : 0;           // first row of the block's picture
  const bool L = (x0 == 0), R = (x1 == pw - 1), T = (y0 == top), B = (y1 == top + ph - 1);
  int16_t* pt = p00 + (size_t)top * stride;                               // sample (0,0) of that picture: the replicas above and below it are written relative to it
  auto val = [&](int r, int cidx) -> int16_t { return PACKED ? src[r * s + cidx] : src[(size_t)(y0 + r) * src_pitch + x0 + cidx]; };
  if (L || R) {
    for (int i = threadIdx.x; i < s * m; i += blockDim.x) {
      int r = i / m, k = i - r * m;
      if (L) p00[(size_t)(y0 + r) * stride - m + k] = val(r, 0);
      if (R) p00[(size_t)(y0 + r) * stride + pw + k] = val(r, s - 1);
    }
  }
  if (T || B) {
    for (int i = threadIdx.x; i < s * m; i += blockDim.x) {
      int k = i / s, cidx = i - k * s;
      if (T) pt[-(ptrdiff_t)(k + 1) * stride + x0 + cidx] = val(0, cidx);
      if (B) pt[(size_t)(ph + k) * stride + x0 + cidx] = val(s - 1, cidx);
    }
  }
  if ((L || R) && (T || B)) {
    for (int i = threadIdx.x; i < m * m; i += blockDim.x) {
      int k = i / m, q = i - k * m;
      if (T && L) pt[-(ptrdiff_t)(k + 1) * stride - m + q] = val(0, 0);
      if (T && R) pt[-(ptrdiff_t)(k + 1) * stride + pw + q] = val(0, s - 1);
      if (B && L) pt[(size_t)(ph + k) * stride - m + q] = val(s - 1, 0);
      if (B && R) pt[(size_t)(ph + k) * stride + pw + q] = val(s - 1, s - 1);
    }
  }
}

