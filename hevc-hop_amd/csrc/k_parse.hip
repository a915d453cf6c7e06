// k_parse.hip -- hop_slice_data_parse: the slice data of the context's picture(s) parsed on the device, the mirror image of hop_slice_data_write (csrc/k_entropy.hip).
// Replaces: the parsing half of TDecSlice::decompressSlice (TLibDecoder/TDecSlice.cpp:108-380) and everything it drives -- the arithmetic decoder, the syntax parsers and
// the derivations are csrc/k_parse_dev.inl (over the tables and helpers of csrc/k_entropy_dev.inl), compiled here for the device and by host/hop_parse.cpp for the host.
//
// Mapping: the arithmetic decoder is serial inside a substream, so ONE WAVE parses one substream and lane 0 does the parsing; the decoder's registers, the 180 context
// models and the current coefficient group live in LDS (ParDec).  Unlike the writer a parser cannot resolve WaveFrontSynchro ahead of time: the CTU at (r, c) needs the
// context models row r - 1 holds after its CTU 1, the depths and skip flags of CTU (r - 1, c) and the vectors of (r - 1, c) and (r - 1, c + 1).  So the rows advance in
// DIAGONAL LAUNCHES: launch d parses CTU c = d - 2 r of every row r that has one, of all pictures of a stack side by side, with only those rows in the grid --
// wctu + 2 (hctu - 1) launches.  Between launches a substream's decoder rests in global memory (ParState, 204 bytes); the other lanes of the wave move it in and out,
// with both barriers outside lane-divergent code.  Without wpp one launch and one wave per picture walk all CTUs.
//   k_parse_init   every unit of the outputs as an unparsed one (what a substream that stops early leaves behind)
//   k_parse_diag   one wave per active row: load, one CTU, store; the models after CTU 1 become the next row's entry state
// No kernel looks at another workgroup's progress.  As in the writer, the pictures of a stack may differ in their slice QP: one table of initial models per distinct QP,
// and a picture's rows start from the table init_of names for it (indexed by the block's picture, wave-uniform).
#include <algorithm>
#include <vector>
#include "hop_dev.h"

#define ENT_FN __device__ static
#define ENT_TAB __constant__ static const
#include "k_entropy_dev.inl"
#include "k_parse_dev.inl"

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hop_set_err((c), HOP_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

extern "C" {
int hop_ent_init_states(uint8_t st[EN_STATES], int slice_type, int qp);                                            // host/hop_entropy.cpp
int hop_parse_check(int pic_w, int pic_h, int bit_depth, int n_pic, const hop_slice_data_params* p, const uint8_t* data, const uint32_t* substream_bytes, int n_substreams,
                    const hop_cu_part* parts, const hop_sao_param* sao, size_t* total, char* err, size_t errn);     // host/hop_parse.cpp
__attribute__((visibility("hidden"))) int hop_parse_device(hop_ctx* c, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data, const uint32_t* substream_bytes,
                                                           int32_t n_substreams, hop_cu_part* parts, int32_t* levels, hop_sao_param* sao, size_t front, const int32_t* pic_qp);
struct hop_parse_where { const hop_cu_part* d_parts; const int32_t* d_levels; size_t end; };   // where the parser left its outputs on the device; the end of its work area
__attribute__((visibility("hidden"))) int hop_parse_device_at(hop_ctx* c, const char* who, const char* noun, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data,
                                                              const unsigned long long* offsets, const uint32_t* substream_bytes, int32_t n_substreams, hop_cu_part* parts,
                                                              int32_t* levels, hop_sao_param* sao, size_t front, hop_parse_where* where, const int32_t* pic_qp);
}

namespace {
struct ParState { uint32_t range, value; int32_t bits_needed; uint32_t pos, flags; int32_t err_ctu; uint32_t st[EN_STATES / 4]; };   // a substream's decoder between two launches
struct ParArgs {
  ParPic pic;                      // parts / levels / sao: picture 0's
  int32_t n_pic, n_sub;
  const uint8_t* init;             // EN_STATES per distinct QP: the initial context models
  const int32_t* init_of;          // per picture: which of them (NULL: one QP, table 0)
  uint8_t* entry;                  // wpp: EN_STATES per CTU row of every picture
  const uint8_t* data; const unsigned long long* offs; const uint32_t* sizes;   // per substream: where its bytes start, how many they are
  ParState* state;                 // per substream
};
static_assert(EN_STATES % 4 == 0 && offsetof(ParDec, st) % 4 == 0, "the context models move as words");

__device__ static inline ParPic par_picture(const ParArgs& A, int k) {
  ParPic g = A.pic;
  const size_t n = (size_t)g.e.wctu * g.e.hctu;
  g.parts += (size_t)k * n * 256; g.e.parts = g.parts;
  if (g.levels) { g.levels += (size_t)k * n * 6144; g.e.levels = g.levels; }
  if (g.sao) { g.sao += (size_t)k * n * 3; g.e.sao = g.sao; }
  return g;
}

__global__ __launch_bounds__(256) void k_parse_init(hop_cu_part* parts, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) pa_unit_init(parts[i], 0);
}

// launch d of a wavefront picture: block b = (picture, active row); rows r0 .. r0 + n_act - 1 have a CTU on this diagonal.  wpp == 0: d < 0, one block per picture, all CTUs.
__global__ __launch_bounds__(64) void k_parse_diag(ParArgs A, int d, int r0, int n_act) {
  __shared__ ParDec k;
  const int t = threadIdx.x, b = blockIdx.x;
  const int pic = d < 0 ? b : b / n_act, r = d < 0 ? 0 : r0 + (b - pic * n_act), col = d < 0 ? 0 : d - 2 * r;
  const ParPic g = par_picture(A, pic);
  const int sub = pic * A.n_sub + r;
  ParState& S = A.state[sub];
  uint32_t* st = (uint32_t*)k.st;
  if (col == 0) {                                                         // a picture one CTU wide has no CTU above right: every row starts from the initial models
    const uint32_t* e = (const uint32_t*)((r == 0 || g.e.wctu < 2) ? (A.init_of ? A.init + (size_t)A.init_of[pic] * EN_STATES : A.init) : A.entry + ((size_t)pic * g.e.hctu + r) * EN_STATES);
    if (t < EN_STATES / 4) st[t] = e[t];
  } else if (t < EN_STATES / 4) st[t] = S.st[t];
  __syncthreads();
  if (t == 0) {
    if (col == 0) {
      k.data = A.data + A.offs[sub]; k.pos = 0; k.size = A.sizes[sub]; k.flags = 0; k.err_ctu = -1;
      pa_start(k);
    } else {
      k.data = A.data + A.offs[sub]; k.size = A.sizes[sub];
      k.range = S.range; k.value = S.value; k.bits_needed = S.bits_needed; k.pos = S.pos; k.flags = S.flags; k.err_ctu = S.err_ctu;
    }
    if (d < 0) for (int a = 0; a < g.e.wctu * g.e.hctu; a++) pa_parse_ctu(k, g, a);
    else pa_parse_ctu(k, g, r * g.e.wctu + col);
    S.range = k.range; S.value = k.value; S.bits_needed = k.bits_needed; S.pos = k.pos; S.flags = k.flags; S.err_ctu = k.err_ctu;
  }
  __syncthreads();
  if (t < EN_STATES / 4) {
    S.st[t] = st[t];
    if (d >= 0 && col == 1 && r + 1 < g.e.hctu) ((uint32_t*)(A.entry + ((size_t)pic * g.e.hctu + r + 1) * EN_STATES))[t] = st[t];
  }
}
}  // namespace

// the work area: the outputs, the models, the substreams' places and states, and (when the data comes from the host) the data
struct ParLayout { size_t o_parts, o_levels, o_sao, o_init, o_init_of, o_entry, o_offs, o_sizes, o_state, o_data, end; };
static ParLayout par_layout(size_t front, int n_pic, int n, int hctu, int n_blocks, bool with_levels, bool with_sao, size_t own_data, int n_init /* tables of initial models */) {
  ParLayout L;
  size_t end = front;
  auto seg = [&](size_t bytes) { const size_t at = (end + 255) & ~(size_t)255; end = at + bytes; return at; };
  L.o_parts = seg(sizeof(hop_cu_part) * 256 * (size_t)n * n_pic); L.o_levels = seg(with_levels ? sizeof(int32_t) * 6144 * (size_t)n * n_pic : 0);
  L.o_sao = seg(with_sao ? sizeof(hop_sao_param) * 3 * (size_t)n * n_pic : 0); L.o_init = seg((size_t)n_init * EN_STATES); L.o_init_of = seg(sizeof(int32_t) * (size_t)n_pic); L.o_entry = seg((size_t)n_pic * hctu * EN_STATES);
  L.o_offs = seg(sizeof(unsigned long long) * n_blocks); L.o_sizes = seg(sizeof(uint32_t) * n_blocks); L.o_state = seg(sizeof(ParState) * n_blocks); L.o_data = seg(own_data);
  L.end = end;
  return L;
}

// internal: an upper bound of what hop_parse_device adds to the scratch area behind `front` bytes of its caller's, for the picture(s) of the context, n_substreams each
extern "C" __attribute__((visibility("hidden"))) size_t hop_parse_work_bytes(const hop_ctx* c, size_t data_bytes, int n_substreams) {
  const int n_pic = c->sub_pitch ? (c->pic_h - c->sub_h) / c->sub_pitch + 1 : 1, ph = c->sub_pitch ? c->sub_h : c->pic_h;
  const int wctu = (c->pic_w + 63) / 64, hctu = (ph + 63) / 64;
  return par_layout(0, n_pic, wctu * hctu, hctu, n_pic * n_substreams, true, true, data_bytes + 256, n_pic).end + 256;   // (at most one table of initial models per picture)
}

extern "C" int hop_slice_data_parse(hop_ctx* c, const hop_slice_data_params* p, const uint8_t* data, const uint32_t* substream_bytes, int32_t n_substreams,
                                    hop_cu_part* parts, int32_t* levels, hop_sao_param* sao) {
  if (!c || !p || !data || !substream_bytes || !parts) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_parse: bad argument");
  return hop_parse_device(c, p, data, nullptr, substream_bytes, n_substreams, parts, levels, sao, 0, hop_picture_qps(c));
}

// internal: the parser over substreams that are on the host (data) or already on the device (d_data, inside the first `front` bytes of the context's scratch area, which
// the caller sized with hop_parse_work_bytes so that it does not move here): hop_access_unit_decode hands over what its compact kernel wrote.  pic_qp (host, one per
// picture of the context) or NULL: p->qp for all pictures
extern "C" __attribute__((visibility("hidden"))) int hop_parse_device(hop_ctx* c, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data, const uint32_t* substream_bytes, int32_t n_substreams,
                                hop_cu_part* parts, int32_t* levels, hop_sao_param* sao, size_t front, const int32_t* pic_qp) {
  return hop_parse_device_at(c, "hop_slice_data_parse", "picture", p, data, d_data, nullptr, substream_bytes, n_substreams, parts, levels, sao, front, nullptr, pic_qp);
}

// internal: the same with the substreams wherever they lie -- offsets (host, may be NULL: back to back): where substream i starts, counted from d_data, all of it inside
// the first `front` bytes of the scratch area -- and with the outputs left in the work area for the next kernels: `where` (may be NULL) says where.  With `where` the
// levels are parsed into the work area also when `levels` is NULL: hop_access_units_decode (csrc/k_stream.hip) hands them to k_dec_ctu where they lie and downloads them
// only for a caller who asks.  who / noun: how an error names the entry and a picture ("picture", "access unit").
extern "C" __attribute__((visibility("hidden"))) int hop_parse_device_at(hop_ctx* c, const char* who, const char* noun, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data,
                                const unsigned long long* offsets, const uint32_t* substream_bytes, int32_t n_substreams, hop_cu_part* parts, int32_t* levels, hop_sao_param* sao,
                                size_t front, hop_parse_where* where, const int32_t* pic_qp) {
  if (!c || !p || (!data && !d_data) || (offsets && !d_data) || !substream_bytes || !parts) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_parse: bad argument");
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_parse: a sharded context parses no slice data");
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_parse: luma and chroma bit depths differ");
  const int n_pic = c->sub_pitch ? (c->pic_h - c->sub_h) / c->sub_pitch + 1 : 1, ph = c->sub_pitch ? c->sub_h : c->pic_h;
  char err[256]; size_t total = 0;
  int r = hop_parse_check(c->pic_w, ph, c->bd_y, n_pic, p, data ? data : d_data, substream_bytes, n_substreams, parts, sao, &total, err, sizeof(err));
  if (r) return hop_set_err(c, r, "%s", err);
  std::vector<uint8_t> init; std::vector<int32_t> init_of;
  if (hop_ent_init_tables(p->slice_type, p->qp, pic_qp, n_pic, init, init_of)) return hop_set_err(c, HOP_ERR_ARG, "hop_slice_data_parse: slice type %d, or a picture's qp outside 0..51", p->slice_type);
  const int wctu = (c->pic_w + 63) / 64, hctu = (ph + 63) / 64, n = wctu * hctu;
  const int n_sub = n_substreams, n_blocks = n_pic * n_sub;
  std::vector<unsigned long long> offs((size_t)n_blocks);
  { unsigned long long at = 0; for (int i = 0; i < n_blocks; i++) { offs[i] = offsets ? offsets[i] : at; at += substream_bytes[i]; } }
  const bool dev_levels = levels != nullptr || where != nullptr;
  const size_t units = (size_t)n * n_pic * 256, parts_bytes = sizeof(hop_cu_part) * units, level_bytes = dev_levels ? sizeof(int32_t) * 6144 * (size_t)n * n_pic : 0,
               sao_bytes = sao ? sizeof(hop_sao_param) * 3 * (size_t)n * n_pic : 0;
  const ParLayout L = par_layout(front, n_pic, n, hctu, n_blocks, dev_levels, sao != nullptr, d_data ? 0 : total + 256, (int)(init.size() / EN_STATES));
  const size_t o_parts = L.o_parts, o_levels = L.o_levels, o_sao = L.o_sao, o_init = L.o_init, o_init_of = L.o_init_of, o_entry = L.o_entry, o_offs = L.o_offs, o_sizes = L.o_sizes, o_state = L.o_state,
               o_data = L.o_data;
  if (d_data && (!c->scratch || L.end > c->scratch_bytes)) return hop_set_err(c, HOP_ERR_STATE, "hop_slice_data_parse: the caller's scratch area of %zu bytes does not hold %zu", c->scratch_bytes, L.end);
  void* buf; r = hop_scratch(c, L.end, &buf); if (r) return r;
  char* b = (char*)buf;
  if (offsets) {                                                           // every substream inside the caller's part of the scratch area
    const size_t base = (size_t)((const char*)d_data - b);
    for (int i = 0; i < n_blocks; i++)
      if ((const char*)d_data < b || base + offs[i] + substream_bytes[i] > front) return hop_set_err(c, HOP_ERR_STATE, "%s: substream %d lies outside the caller's %zu bytes", who, i, front);
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_data) HIPCHK(c, hipMemcpyAsync(b + o_data, data, total, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_init, init.data(), init.size(), hipMemcpyHostToDevice, c->stream));
  if (!init_of.empty()) HIPCHK(c, hipMemcpyAsync(b + o_init_of, init_of.data(), sizeof(int32_t) * init_of.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_offs, offs.data(), sizeof(unsigned long long) * n_blocks, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_sizes, substream_bytes, sizeof(uint32_t) * n_blocks, hipMemcpyHostToDevice, c->stream));
  if (dev_levels) HIPCHK(c, hipMemsetAsync(b + o_levels, 0, level_bytes, c->stream));   // lane 0 stores the non-zero levels only
  if (sao) HIPCHK(c, hipMemsetAsync(b + o_sao, 0, sao_bytes, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_state, 0, sizeof(ParState) * n_blocks, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_entry, 0, (size_t)n_pic * hctu * EN_STATES, c->stream));
  ParArgs A;
  A.pic.e.pic_w = c->pic_w; A.pic.e.pic_h = ph; A.pic.e.wctu = wctu; A.pic.e.hctu = hctu;
  A.pic.e.i_slice = p->slice_type == 2; A.pic.e.sao_luma = p->sao_luma; A.pic.e.sao_chroma = p->sao_chroma; A.pic.e.sao_max_offset = (1 << (std::min(c->bd_y, 10) - 5)) - 1;
  A.pic.parts = (hop_cu_part*)(b + o_parts); A.pic.levels = dev_levels ? (int32_t*)(b + o_levels) : nullptr; A.pic.sao = sao ? (hop_sao_param*)(b + o_sao) : nullptr;
  if (where) { where->d_parts = A.pic.parts; where->d_levels = A.pic.levels; where->end = L.end; }
  A.pic.e.parts = A.pic.parts; A.pic.e.levels = A.pic.levels; A.pic.e.sao = A.pic.sao; A.pic.e.scans = c->rdoq_scans;
  A.pic.wpp = p->wpp; A.pic.sao_shift = c->bd_y - std::min(c->bd_y, 10); A.pic.mi_size = p->mi_size; A.pic.mi_merge = !p->plain_intra;
  A.n_pic = n_pic; A.n_sub = n_sub;
  A.init = (const uint8_t*)(b + o_init); A.init_of = init_of.empty() ? nullptr : (const int32_t*)(b + o_init_of); A.entry = (uint8_t*)(b + o_entry);
  A.data = d_data ? d_data : (const uint8_t*)(b + o_data); A.offs = (const unsigned long long*)(b + o_offs); A.sizes = (const uint32_t*)(b + o_sizes);
  A.state = (ParState*)(b + o_state);
  hipLaunchKernelGGL(k_parse_init, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, c->stream, A.pic.parts, units);
  if (!p->wpp) {
    const int pr = hop_prof_begin(c, HOP_K_PARSE, (uint64_t)n_pic * n);
    hipLaunchKernelGGL(k_parse_diag, dim3(n_pic), dim3(64), 0, c->stream, A, -1, 0, 1);
    hop_prof_end(c, pr);
  } else {
    for (int d = 0; d < wctu + 2 * (hctu - 1); d++) {                     // row r is at column d - 2 r
      const int r0 = std::max(0, (d - wctu + 2) / 2), r1 = std::min(hctu - 1, d / 2), n_act = r1 - r0 + 1;
      if (n_act <= 0) continue;                                             // a picture one CTU wide has nothing on its odd diagonals
      const int pr = hop_prof_begin(c, HOP_K_PARSE, (uint64_t)n_pic * n_act);
      hipLaunchKernelGGL(k_parse_diag, dim3(n_pic * n_act), dim3(64), 0, c->stream, A, d, r0, n_act);
      hop_prof_end(c, pr);
    }
  }
  hipError_t e = hipGetLastError();
  std::vector<ParState> st((size_t)n_blocks);
  if (e == hipSuccess) e = hipMemcpyAsync(st.data(), A.state, sizeof(ParState) * n_blocks, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(parts, b + o_parts, parts_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && levels) e = hipMemcpyAsync(levels, b + o_levels, level_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && sao) e = hipMemcpyAsync(sao, b + o_sao, sao_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  for (int i = 0; i < n_blocks; i++) {
    const uint32_t f = st[i].flags;
    if (!f) continue;
    const int first = p->wpp ? (i % n_sub) * wctu : 0;
    return hop_set_err(c, HOP_ERR_ARG, "%s: substream %d of %s %d, CTU %d: %s (%u of %u bytes consumed)", who, i % n_sub, noun, i / n_sub,
                       st[i].err_ctu < 0 ? first : st[i].err_ctu,
                       (f & PA_ERR_END) ? "the stream ran past the substream's end" : (f & PA_ERR_RANGE) ? "a value out of range" : "a terminating bin or the consumed length is wrong",
                       st[i].pos, substream_bytes[i]);
  }
  return HOP_OK;
}
