// k_entropy.hip -- hop_slice_data_write: the slice data of the context's picture(s) coded on the device.
// Replaces: TEncSlice::encodeSlice (TLibEncoder/TEncSlice.cpp:1228-1500) and everything it drives -- the syntax walk and the arithmetic coder are csrc/k_entropy_dev.inl,
// compiled here for the device and by host/hop_entropy.cpp for the host.
//
// Mapping: the arithmetic coder is serial inside a substream and the substreams are independent, so ONE WAVE codes one substream and lane 0 does the coding; the coder's
// registers and the 180 context models live in LDS (EntCoder), the bytes leave through ordinary stores into the substream's own slab.  WaveFrontSynchro makes row r + 1
// start from the context models row r holds after its second CTU; that chain needs no arithmetic coder, so it is resolved by a launch of its own instead of a wait:
//   k_entropy_context  one wave per picture: rows 0 .. R-2 in order, the first two CTUs of each with the bins moving the context models only; the models after the second
//                      CTU are stored as the next row's entry state (a picture one CTU wide: every row starts from the initial models)
//   k_entropy_code     one wave per substream of every picture, each from its entry state: SAO parameters, coding quadtree, terminating bins, finish, byte alignment
//   k_entropy_pack     the substreams copied back to back (each block sums the sizes in front of its own), so that one transfer brings them to the host
// No kernel looks at another workgroup's progress.  The pictures of a stack may differ in their slice QP (hop_ctx_set_picture_qps): one table of initial models per
// distinct QP is uploaded once per call, and a picture's waves start from the table init_of names for it -- an index by the block's picture, wave-uniform.
#include <algorithm>
#include <vector>
#include "hop_dev.h"

#define ENT_FN __device__ static
#define ENT_TAB __constant__ static const
#include "k_entropy_dev.inl"

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hop_set_err((c), HOP_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

extern "C" {
int hop_ent_init_states(uint8_t st[EN_STATES], int slice_type, int qp);                                            // host/hop_entropy.cpp
int hop_ent_check(int pic_w, int pic_h, int bit_depth, int n_pic, const hop_slice_data_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao,
                  char* err, size_t errn);
}

namespace {
struct EntArgs {
  EntPic pic;                      // parts / levels / sao: picture 0's
  int32_t n_pic, n_sub, wpp;
  size_t level_pic_stride;         // TCoeff between the levels of two pictures
  const uint8_t* init;             // EN_STATES per distinct QP: the initial context models
  const int32_t* init_of;          // per picture: which of them (NULL: one QP, table 0)
  uint8_t* entry;                  // wpp: EN_STATES per CTU row of every picture
  uint8_t* slabs; size_t slab_stride; uint32_t slab_limit;   // a slab per substream; bytes are stored below slab_limit only
  uint32_t* sizes; uint32_t* flags;                          // per substream: its length; bit 0 a byte did not fit, bit 1 data without syntax
};

__device__ static inline EntPic ent_picture(const EntArgs& A, int k) {
  EntPic g = A.pic;
  const size_t n = (size_t)g.wctu * g.hctu;
  g.parts += (size_t)k * n * 256; g.levels += (size_t)k * A.level_pic_stride;
  if (g.sao) g.sao += (size_t)k * n * 3;
  return g;
}

__device__ static inline const uint8_t* ent_init(const EntArgs& A, int k) { return A.init_of ? A.init + (size_t)A.init_of[k] * EN_STATES : A.init; }

__global__ __launch_bounds__(64) void k_entropy_context(EntArgs A) {
  __shared__ EntCoder k;
  if (threadIdx.x != 0) return;                                          // no barrier in this kernel
  const EntPic g = ent_picture(A, blockIdx.x);
  en_context_pass(k, g, ent_init(A, blockIdx.x), A.entry + (size_t)blockIdx.x * g.hctu * EN_STATES);
}

__global__ __launch_bounds__(64) void k_entropy_code(EntArgs A) {
  __shared__ EntCoder k;
  if (threadIdx.x != 0) return;                                          // no barrier in this kernel
  const int b = blockIdx.x, pic = b / A.n_sub, s = b - pic * A.n_sub;
  const EntPic g = ent_picture(A, pic);
  const uint8_t* entry = A.wpp ? A.entry + ((size_t)pic * g.hctu + s) * EN_STATES : ent_init(A, pic);
  en_code_substream(k, g, entry, A.wpp ? s * g.wctu : 0, A.wpp ? g.wctu : g.wctu * g.hctu, A.slabs + (size_t)b * A.slab_stride, A.slab_limit);
  A.sizes[b] = k.pos;
  A.flags[b] = (k.overflow ? 1u : 0u) | (k.error ? 2u : 0u);
}

__global__ __launch_bounds__(256) void k_entropy_pack(const uint8_t* __restrict__ slabs, size_t slab_stride, uint32_t slab_limit, const uint32_t* __restrict__ sizes,
                                                      uint8_t* __restrict__ dst, size_t capacity) {
  __shared__ unsigned long long part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  unsigned long long s = 0;
  for (int i = t; i < b; i += 256) s += sizes[i];
  part[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (t < o) part[t] += part[t + o]; __syncthreads(); }
  const size_t off = (size_t)part[0];
  const uint32_t n = sizes[b] < slab_limit ? sizes[b] : slab_limit;       // what the slab holds
  const uint8_t* src = slabs + (size_t)b * slab_stride;
  for (uint32_t i = t; i < n; i += 256) if (off + i < capacity) dst[off + i] = src[i];
}
}  // namespace

// internal (hop_dev.h): the initial context models of the pictures of a call -- one table per distinct QP in `tabs`, picture k's in table init_of[k].  pic_qp == NULL: one
// table at `qp`, init_of left empty (the kernels then take table 0 without looking).  Returns non-zero for a slice type that has no models.
int hop_ent_init_tables(int slice_type, int qp, const int32_t* pic_qp, int n_pic, std::vector<uint8_t>& tabs, std::vector<int32_t>& init_of) {
  tabs.clear(); init_of.clear();
  if (!pic_qp) { tabs.resize(EN_STATES); return hop_ent_init_states(tabs.data(), slice_type, qp); }
  std::vector<int32_t> at(52, -1);
  for (int k = 0; k < n_pic; k++) {
    const int q = pic_qp[k];
    if (q < 0 || q > 51) return 1;
    if (at[q] < 0) {
      at[q] = (int32_t)(tabs.size() / EN_STATES);
      tabs.resize(tabs.size() + EN_STATES);
      if (hop_ent_init_states(tabs.data() + (size_t)at[q] * EN_STATES, slice_type, q)) return 1;
    }
    init_of.push_back(at[q]);
  }
  return 0;
}

// internal: hop_slice_data_write, and for hop_access_unit_write (csrc/k_stream.hip) the same with the substreams LEFT ON THE DEVICE: with d_packed the packed substreams
// are not copied to `out` (which may be NULL) but their device address is returned, with `reserve` further bytes of the same scratch allocation behind them (*d_reserve,
// 256-aligned) -- both valid until the context's scratch area is asked for again.  pic_qp (host, one per picture of the context) or NULL: p->qp for all pictures.
extern "C" __attribute__((visibility("hidden"))) int hop_ent_write_device(hop_ctx* c, const hop_slice_data_params* p, const hop_cu_part* parts, const int32_t* levels,
                                                                         const hop_sao_param* sao, uint8_t* out, size_t out_capacity, uint32_t* substream_bytes,
                                                                         int32_t* n_substreams, size_t reserve, const uint8_t** d_packed, uint8_t** d_reserve,
                                                                         const int32_t* pic_qp) {
  if (!c || !p || !parts || !substream_bytes || !n_substreams || (!out && out_capacity && !d_packed)) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: bad argument");
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: a sharded context writes no slice data");
  if (!levels && !(c->coefpic && c->levels_valid))
    return hop_set_err(c, HOP_ERR_STATE, "hop_slice_data_write: levels == NULL, but the context holds no levels of a finished hop_encode_frame (none has run, the last one failed, or hop_decode_frame has replaced the picture since: pass the levels)");
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: luma and chroma bit depths differ");
  const int n_pic = c->sub_pitch ? (c->pic_h - c->sub_h) / c->sub_pitch + 1 : 1, ph = c->sub_pitch ? c->sub_h : c->pic_h;
  char err[256];
  int r = hop_ent_check(c->pic_w, ph, c->bd_y, n_pic, p, parts, levels, sao, err, sizeof(err));
  if (r) return hop_set_err(c, r, "%s", err);
  std::vector<uint8_t> init; std::vector<int32_t> init_of;
  if (hop_ent_init_tables(p->slice_type, p->qp, pic_qp, n_pic, init, init_of)) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: slice type %d, or a picture's qp outside 0..51", p->slice_type);
  const int wctu = (c->pic_w + 63) / 64, hctu = (ph + 63) / 64, n = wctu * hctu;
  const int n_sub = p->wpp ? hctu : 1, n_blocks = n_pic * n_sub;
  // a substream's slab: what its CTUs can come to at most (per level at most 34 bypass bins and 4 context-coded bins of under 8 bits: 7 bytes; 6144 levels and the CU
  // syntax per CTU: 48 KiB), and never more than the caller's bound
  const size_t bound = (size_t)(p->wpp ? wctu : n) * 49152 + 256;
  const uint32_t slab_limit = (uint32_t)std::min<size_t>(std::min(bound, out_capacity), 0xFFFFFFF0u);
  const size_t slab_stride = ((size_t)slab_limit + 255) & ~(size_t)255, packed = std::min(out_capacity, (size_t)n_blocks * slab_limit);
  size_t end = 0;
  auto seg = [&](size_t bytes) { const size_t at = (end + 255) & ~(size_t)255; end = at + bytes; return at; };
  const size_t o_parts = seg(sizeof(hop_cu_part) * 256 * (size_t)n * n_pic), o_levels = seg(levels ? sizeof(int32_t) * 6144 * (size_t)n * n_pic : 0),
               o_sao = seg(sao ? sizeof(hop_sao_param) * 3 * (size_t)n * n_pic : 0), o_init = seg(init.size()), o_init_of = seg(sizeof(int32_t) * init_of.size()), o_entry = seg((size_t)n_pic * hctu * EN_STATES),
               o_sizes = seg(sizeof(uint32_t) * 2 * (size_t)n_blocks), o_slabs = seg(slab_stride * n_blocks + 256), o_packed = seg(packed + 256), o_reserve = seg(reserve);
  void* buf; r = hop_scratch(c, end, &buf); if (r) return r;
  char* b = (char*)buf;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b + o_parts, parts, sizeof(hop_cu_part) * 256 * (size_t)n * n_pic, hipMemcpyHostToDevice, c->stream));
  if (levels) HIPCHK(c, hipMemcpyAsync(b + o_levels, levels, sizeof(int32_t) * 6144 * (size_t)n * n_pic, hipMemcpyHostToDevice, c->stream));
  if (sao) HIPCHK(c, hipMemcpyAsync(b + o_sao, sao, sizeof(hop_sao_param) * 3 * (size_t)n * n_pic, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_init, init.data(), init.size(), hipMemcpyHostToDevice, c->stream));
  if (!init_of.empty()) HIPCHK(c, hipMemcpyAsync(b + o_init_of, init_of.data(), sizeof(int32_t) * init_of.size(), hipMemcpyHostToDevice, c->stream));
  EntArgs A;
  A.pic.pic_w = c->pic_w; A.pic.pic_h = ph; A.pic.wctu = wctu; A.pic.hctu = hctu;
  A.pic.i_slice = p->slice_type == 2; A.pic.sao_luma = p->sao_luma; A.pic.sao_chroma = p->sao_chroma; A.pic.sao_max_offset = (1 << (std::min(c->bd_y, 10) - 5)) - 1;
  A.pic.parts = (const hop_cu_part*)(b + o_parts);
  // resident levels: picture k's CTUs start at CTU row k * sub_pitch / 64 of the stack's grid (hop_levels_download)
  A.pic.levels = levels ? (const int32_t*)(b + o_levels) : c->coefpic;
  A.level_pic_stride = levels ? (size_t)n * 6144 : (size_t)(c->sub_pitch >> 6) * wctu * 6144;
  A.pic.sao = sao ? (const hop_sao_param*)(b + o_sao) : nullptr;
  A.pic.scans = c->rdoq_scans;
  A.n_pic = n_pic; A.n_sub = n_sub; A.wpp = p->wpp;
  A.init = (const uint8_t*)(b + o_init); A.init_of = init_of.empty() ? nullptr : (const int32_t*)(b + o_init_of); A.entry = (uint8_t*)(b + o_entry);
  A.slabs = (uint8_t*)(b + o_slabs); A.slab_stride = slab_stride; A.slab_limit = slab_limit;
  A.sizes = (uint32_t*)(b + o_sizes); A.flags = A.sizes + n_blocks;
  // (with hop_profile_enable on, the context pass and the coding pass are timed apart: HOP_K_ENTROPY_CTX, HOP_K_ENTROPY)
  if (p->wpp) {
    const int pr = hop_prof_begin(c, HOP_K_ENTROPY_CTX, (uint64_t)n_pic * (hctu - 1) * (wctu < 2 ? 0 : 2));
    hipLaunchKernelGGL(k_entropy_context, dim3(n_pic), dim3(64), 0, c->stream, A);
    hop_prof_end(c, pr);
  }
  {
    const int pr = hop_prof_begin(c, HOP_K_ENTROPY, (uint64_t)n_pic * n);
    hipLaunchKernelGGL(k_entropy_code, dim3(n_blocks), dim3(64), 0, c->stream, A);
    hop_prof_end(c, pr);
  }
  hipLaunchKernelGGL(k_entropy_pack, dim3(n_blocks), dim3(256), 0, c->stream, (const uint8_t*)A.slabs, slab_stride, slab_limit, (const uint32_t*)A.sizes, (uint8_t*)(b + o_packed), packed);
  hipError_t e = hipGetLastError();
  std::vector<uint32_t> sz(2 * (size_t)n_blocks);
  if (e == hipSuccess) e = hipMemcpyAsync(sz.data(), A.sizes, sizeof(uint32_t) * 2 * (size_t)n_blocks, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "hop_slice_data_write: %s", hipGetErrorString(e));
  size_t total = 0; bool bad = false;
  for (int i = 0; i < n_blocks; i++) { substream_bytes[i] = sz[i]; total += sz[i]; bad = bad || (sz[n_blocks + i] & 2u); }
  if (bad) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: the levels contradict the partition data (a coded block without a level, or a level beyond 16 bits)");
  if (total > out_capacity) {
    *n_substreams = (int32_t)std::min<size_t>(total, 0x7FFFFFFF);
    return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_write: the slice data takes %zu bytes, out_capacity is %zu", total, out_capacity);
  }
  for (int i = 0; i < n_blocks; i++) if ((sz[n_blocks + i] & 1u) || sz[i] > slab_limit) return hop_set_err(c, HOP_ERR_DEVICE, "hop_slice_data_write: substream %d outgrew its slab (%u bytes)", i, sz[i]);
  if (d_packed) { *d_packed = (const uint8_t*)(b + o_packed); *d_reserve = (uint8_t*)(b + o_reserve); }
  else if (total) HIPCHK(c, hipMemcpy(out, b + o_packed, total, hipMemcpyDeviceToHost));
  *n_substreams = n_sub;
  return HOP_OK;
}

extern "C" int hop_slice_data_write(hop_ctx* c, const hop_slice_data_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao,
                                    uint8_t* out, size_t out_capacity, uint32_t* substream_bytes, int32_t* n_substreams) {
  return hop_ent_write_device(c, p, parts, levels, sao, out, out_capacity, substream_bytes, n_substreams, 0, nullptr, nullptr, c ? hop_picture_qps(c) : nullptr);
}
