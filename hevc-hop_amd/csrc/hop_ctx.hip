// hop_ctx.hip -- context, picture residency, host-side logic and the C ABI glue of libhophip.so.
// gfx950 only.  No CPU compute path exists in this library: every hot-path entry point launches a
// HIP kernel and fails with HOP_ERR_DEVICE when there is no device.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <functional>
#include <utility>
#include <algorithm>
#include "hop_dev.h"

static char g_create_err[512] = "";

int hop_set_err(hop_ctx* c, int code, const char* fmt, ...) {
  char* dst = c ? c->err : g_create_err;
  va_list ap; va_start(ap, fmt); vsnprintf(dst, 512, fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  return hop_set_err((c), HOP_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// ---------------------------------------------------------------------------------------------
// what the entry points below share: device buffers that grow on demand, the lanes, the staging arena of the host-array entries, grouping jobs by class, the validators
// ---------------------------------------------------------------------------------------------
// Makes *buf hold at least `need` bytes.  When it has to grow, the stream is synchronised first (queued kernels may still use the old block) and need + slack bytes are allocated.
static int hop_reserve(hop_ctx* c, void** buf, size_t* have, size_t need, size_t slack) {
  if (need <= *have) return HOP_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (*buf) HIPCHK(c, hipFree(*buf));
  *buf = nullptr; *have = 0;
  HIPCHK(c, hipSetDevice(c->device));                                    // (the calling thread's current device may be another context's)
  HIPCHK(c, hipMalloc(buf, need + slack));
  *have = need + slack;
  return HOP_OK;
}
int hop_scratch(hop_ctx* c, size_t bytes, void** out) {
  int r = hop_reserve(c, &c->scratch, &c->scratch_bytes, bytes, bytes / 4 + 4096); if (r) return r;
  *out = c->scratch;
  return HOP_OK;
}
static int hop_stage(hop_ctx* c, size_t bytes, void** out) {
  int r = hop_reserve(c, &c->stage, &c->stage_bytes, bytes, bytes / 4 + 4096); if (r) return r;
  *out = c->stage;
  return HOP_OK;
}
// the quadtree searches' state buffer; it is free again once a search's kernels are queued (same stream), so the stages of a chain share it
static int rqt_reserve(hop_ctx* c, size_t bytes) { return hop_reserve(c, &c->rqt_buf, &c->rqt_bytes, bytes, bytes / 8); }
static int walk_reserve(hop_ctx* c, size_t bytes) { return hop_reserve(c, &c->walk_buf, &c->walk_bytes, bytes, bytes / 4); }

// The streams and events of a context: its own stream, the extra lanes' streams and join events, the fork event.
// The context's own stream -- the spine's short requests: predictions, searches, block copies -- runs at the highest priority, the views' streams (the candidate
// evaluations, hundreds of long workgroups in flight) at the lowest: without it a 10 us prediction kernel waits for a free compute unit behind them (measured on the
// 7728-wide picture: 0.15 ms -> 0.03 ms per prediction request, 27 -> 35 CTU/s).  HOP_STREAM_PRIO=0 turns it off.
static hipError_t create_stream(hipStream_t* out, unsigned stream_flags, bool highest_priority) {
  int prio_lo = 0, prio_hi = 0; (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  const char* f = getenv("HOP_STREAM_PRIO");
  return (f && f[0] == '0') ? hipStreamCreateWithFlags(out, stream_flags) : hipStreamCreateWithPriority(out, stream_flags, highest_priority ? prio_hi : prio_lo);
}
// (borrowed: the context's own stream is that one, hop_ctx_create_view_on)
static hipError_t create_lanes(hop_ctx* c, unsigned stream_flags, bool highest_priority, hipStream_t borrowed = nullptr) {
  hipError_t e = hipSuccess;
  if (borrowed) { c->stream = borrowed; c->borrowed_stream = true; } else e = create_stream(&c->stream, stream_flags, highest_priority);
  for (int k = 0; k < HOP_MAX_LANES - 1 && e == hipSuccess; k++) {
    e = hipStreamCreateWithFlags(&c->xlane[k].stream, stream_flags);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  return e;
}

// While it lives the context works on extra lane k: that lane's stream and work areas stand in for the context's own.
struct lane_scope {
  hop_lane &own, &other;
  lane_scope(hop_ctx* c, int k) : own(*c), other(c->xlane[k]) { std::swap(own, other); }
  ~lane_scope() { std::swap(own, other); }
  lane_scope(const lane_scope&) = delete;
};

// body(0) .. body(n_items - 1), item i on lane i % HOP_MAX_LANES: the items are independent chains of kernels, each lane a stream with work areas of its own.  The extra
// lanes this call uses start behind what is queued on the context's stream, and the stream continues behind them.  Stops issuing at the first item that fails.
template <class Body>
static int run_on_lanes(hop_ctx* c, int n_items, const char* what, Body body) {
  const int n_fork = std::min(n_items, HOP_MAX_LANES) - 1;
  if (n_fork > 0) HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
  for (int k = 0; k < n_fork; k++) HIPCHK(c, hipStreamWaitEvent(c->xlane[k].stream, c->ev_fork, 0));
  bool used[HOP_MAX_LANES - 1] = { false, false, false };
  int rc = HOP_OK;
  for (int i = 0; i < n_items && rc == HOP_OK; i++) {
    const int lane = i % HOP_MAX_LANES;
    if (lane == 0) { rc = body(i); continue; }
    lane_scope on(c, lane - 1);
    rc = body(i);
    used[lane - 1] = true;
  }
  for (int k = 0; k < HOP_MAX_LANES - 1; k++) {
    if (!used[k]) continue;
    hipError_t e = hipEventRecord(c->ev_join[k], c->xlane[k].stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_join[k], 0);
    if (e != hipSuccess && rc == HOP_OK) rc = hop_set_err(c, HOP_ERR_DEVICE, "%s: stream join: %s", what, hipGetErrorString(e));
  }
  return rc;
}

// The staging area of one host-array call.  The entry declares its segments in the order they lie in the area, each 256-byte aligned: in() is uploaded from the host,
// out() is room for results, zero() is room that is cleared; end_mark() is the aligned end.  commit() makes the one reservation (it may reallocate, so nothing is copied
// before it) and issues the uploads and clears on c->stream in the order they were declared.  After it a[seg] is the segment's device pointer, download() copies a segment
// back and sync() waits for the stream.  A segment's type and element count are stated once, at its declaration; every copy takes its size from there.
struct stage_arena {
  template <class T> struct seg { int i; };
  explicit stage_arena(hop_ctx* ctx) : c(ctx) {}
  template <class T> seg<T> out(size_t m) {
    const size_t off = (end + 255) & ~(size_t)255;
    segs.push_back({ off, m * sizeof(T) }); end = off + m * sizeof(T);
    return seg<T>{ (int)segs.size() - 1 };
  }
  template <class T> seg<T> in(const T* src, size_t m) { seg<T> s = out<T>(m); ops.push_back({ s.i, s.i, src }); return s; }
  template <class T> seg<T> zero(size_t m) { seg<T> s = out<T>(m); ops.push_back({ s.i, s.i, nullptr }); return s; }
  seg<char> end_mark() { return out<char>(0); }
  template <class T> void zero_span(seg<T> first, seg<char> last) { ops.push_back({ first.i, last.i, nullptr }); }   // first .. last in one clear, the padding between them included
  int commit(size_t slack) {
    void* st; int r = hop_stage(c, end + slack, &st); if (r) return r;
    base = (char*)st;
    for (const op& o : ops) {
      const extent& s = segs[o.first];
      if (o.src) HIPCHK(c, hipMemcpyAsync(base + s.off, o.src, s.bytes, hipMemcpyHostToDevice, c->stream));
      else HIPCHK(c, hipMemsetAsync(base + s.off, 0, segs[o.last].off + segs[o.last].bytes - s.off, c->stream));
    }
    return HOP_OK;
  }
  template <class T> T* operator[](seg<T> s) const { return (T*)(base + segs[s.i].off); }
  template <class T> int upload(seg<T> s, const T* src) { HIPCHK(c, hipMemcpyAsync(base + segs[s.i].off, src, segs[s.i].bytes, hipMemcpyHostToDevice, c->stream)); return HOP_OK; }   // an in() that is not due at commit()
  template <class T> int download(T* dst, seg<T> s) { HIPCHK(c, hipMemcpyAsync(dst, base + segs[s.i].off, segs[s.i].bytes, hipMemcpyDeviceToHost, c->stream)); return HOP_OK; }
  int sync() { HIPCHK(c, hipStreamSynchronize(c->stream)); return HOP_OK; }
 private:
  struct extent { size_t off, bytes; };
  struct op { int first, last; const void* src; };                      // src: upload segment `first`; no src: clear first .. last
  hop_ctx* c; char* base = nullptr; size_t end = 0;
  std::vector<extent> segs; std::vector<op> ops;
};

// body(idx) once per class of the jobs 0 .. n-1 -- i and k are of one class when same(i, k) --, the classes in the order of their first jobs, idx a class's jobs in ascending order
template <class Same, class Body>
static int for_each_class(int n, Same same, Body body) {
  std::vector<char> done(n, 0);
  for (int first = 0; first < n; first++) {
    if (done[first]) continue;
    std::vector<int> idx;
    for (int i = first; i < n; i++) if (!done[i] && same(first, i)) { done[i] = 1; idx.push_back(i); }
    int r = body(idx); if (r) return r;
  }
  return HOP_OK;
}
// The per-job arrays of a class in class order and back: job i's block is `len` elements at src + off[i] (without off: at src + i * len); packed, block t of the
// class is at t * stride (stride 0: len).
template <class T>
static std::vector<T> gather(const T* src, const std::vector<int>& idx, size_t len = 1, const size_t* off = nullptr) {
  std::vector<T> v(idx.size() * len);
  for (size_t t = 0; t < idx.size(); t++) std::copy_n(src + (off ? off[idx[t]] : idx[t] * len), len, v.begin() + t * len);
  return v;
}
template <class T>
static void scatter(T* dst, const std::vector<int>& idx, const T* v, size_t len = 1, const size_t* off = nullptr, size_t stride = 0) {
  for (size_t t = 0; t < idx.size(); t++) std::copy_n(v + t * (stride ? stride : len), len, dst + (off ? off[idx[t]] : idx[t] * len));
}

// A legal class of CUs: size 8..64, transform sizes 4..32, the smallest transform of the CU within them, at most three levels below the CU and the largest at most one.
static bool rqt_class_ok(const hop_rqt_job& j) {
  return j.log2_cu >= 3 && j.log2_cu <= 6 && j.log2_max_tu >= 2 && j.log2_max_tu <= 5 && j.log2_min_tu_in_cu >= 2 && j.log2_min_tu_in_cu <= j.log2_max_tu &&
         j.log2_cu - j.log2_min_tu_in_cu <= 3 && j.log2_cu - j.log2_max_tu <= 1;
}
// same CU size, transform-tree limits and transform-skip switch: the part of the class key every grouped entry has
static bool same_tree(const hop_rqt_job& a, const hop_rqt_job& b) {
  return a.log2_cu == b.log2_cu && a.log2_max_tu == b.log2_max_tu && a.log2_min_tu_in_cu == b.log2_min_tu_in_cu && !a.use_ts == !b.use_ts;
}
// the CU of a legal size, aligned to it and inside the picture
static bool cu_rect_ok(const hop_ctx* c, const hop_rqt_job& j) {
  if (j.log2_cu < 3 || j.log2_cu > 6) return false;
  const int S = 1 << j.log2_cu;
  return j.x >= 0 && j.y >= 0 && (j.x & (S - 1)) == 0 && (j.y & (S - 1)) == 0 && j.x + S <= c->pic_w && j.y + S <= c->pic_h;
}
static size_t cu_coeffs(int log2_cu) { return ((size_t)3 << (2 * log2_cu)) >> 1; }   // levels of a CU: luma + two chroma blocks
// every state of the coder snapshots (and of the CU-level ones, where the entry takes them) is a CABAC state
static bool ctx_states_ok(hop_ctx* c, int n_ctx, const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in) {
  for (int k = 0; k < n_ctx; k++) {
    for (int i = 0; i < 150; i++) if (ctx_in[k].state[i] > 127) { hop_set_err(c, HOP_ERR_ARG, "context snapshot %d: state %d out of range", k, i); return false; }
    for (int i = 0; cu_ctx_in && i < 19; i++) if (cu_ctx_in[k].state[i] > 127) { hop_set_err(c, HOP_ERR_ARG, "CU context snapshot %d: state %d out of range", k, i); return false; }
  }
  return true;
}
// An intra block of a plane, sh = 0 luma / 1 chroma: size (in the plane's samples) 4..64 / 4..32, its position (in luma samples) on the plane's 4-sample grid, inside the plane.
static bool intra_block_ok(const hop_ctx* c, const hop_intra_job& j, int sh) {
  const int N = j.size, grid = (4 << sh) - 1;
  return (N == 4 || N == 8 || N == 16 || N == 32 || (N == 64 && !sh)) && j.x >= 0 && j.y >= 0 && !(j.x & grid) && !(j.y & grid) &&
         (j.x >> sh) + N <= (c->pic_w >> sh) && (j.y >> sh) + N <= (c->pic_h >> sh);
}
// An available neighbour unit (4 luma samples: 4 / 2 samples of the plane) must lie inside the picture (the reference derives availability from existing CUs): units
// 0 .. 2U-1 up the left edge from below, 2U the corner, 2U+1 .. 4U along the top.  *bad is the first unit that does not.
static bool intra_neighbours_ok(const hop_ctx* c, const hop_intra_job& j, int sh, int* bad) {
  const int unit = 4 >> sh, U = j.size / unit, x = j.x >> sh, y = j.y >> sh, w = c->pic_w >> sh, h = c->pic_h >> sh;
  for (int u = 0; u < 4 * U + 1; u++) if (j.flags[u]) {
    bool ok;
    if (u < 2 * U) ok = x > 0 && y + unit * (2 * U - 1 - u) + unit <= h;
    else if (u == 2 * U) ok = x > 0 && y > 0;
    else ok = y > 0 && x + unit * (u - 2 * U - 1) + unit <= w;
    if (!ok) { *bad = u; return false; }
  }
  return true;
}

// The internal forms of hop_ctx_create_view (hop_dev.h): a view on a borrowed stream, the stream such views borrow, and moving a view to another one.
int hop_view_stream_create(hop_ctx* parent, hipStream_t* out) {
  if (!parent || !out) return hop_set_err(parent, HOP_ERR_ARG, "hop_view_stream_create: bad argument");
  HIPCHK(parent, hipSetDevice(parent->device));
  HIPCHK(parent, create_stream(out, hipStreamNonBlocking, false));
  return HOP_OK;
}
void hop_view_set_stream(hop_ctx* view, hipStream_t borrowed) { if (view && view->borrowed_stream && borrowed) view->stream = borrowed; }
int hop_ctx_create_view_on(hop_ctx* parent, hipStream_t borrowed, hop_ctx** out) {
  if (!parent || !out) return hop_set_err(parent, HOP_ERR_ARG, "hop_ctx_create_view_on: bad argument");       // (a view of a view is one more view of the same pictures)
  *out = nullptr;
  hop_ctx* c = (hop_ctx*)calloc(1, sizeof(hop_ctx));
  c->pic_w = parent->pic_w; c->pic_h = parent->pic_h; c->bd_y = parent->bd_y; c->bd_c = parent->bd_c; c->device = parent->device;
  c->stride_y = parent->stride_y; c->stride_c = parent->stride_c; c->sub_h = parent->sub_h; c->sub_pitch = parent->sub_pitch; c->slots = parent->slots; c->fused_leaf_max = parent->fused_leaf_max; c->walk_max = parent->walk_max; c->ss_families = parent->ss_families; c->row_limit = parent->row_limit; c->lanes = 1; c->is_view = true;
  c->org_y = parent->org_y; c->org_cb = parent->org_cb; c->org_cr = parent->org_cr;
  for (int k = 0; k < 3; k++) { c->ss_alloc[k] = parent->ss_alloc[k]; c->ss_buf[k] = parent->ss_buf[k]; c->ss00[k] = parent->ss00[k]; c->pred[k] = parent->pred[k]; c->rec[k] = parent->rec[k]; }
  c->entropy_bits = parent->entropy_bits; c->rdoq_scans = parent->rdoq_scans; c->have_orig = parent->have_orig; c->stash = parent->stash; c->stash_slots = parent->stash_slots; c->coefpic = parent->coefpic; c->coef_stash = parent->coef_stash; c->pic_qps = parent->pic_qps;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = create_lanes(c, hipStreamNonBlocking, false, borrowed);
  if (e != hipSuccess) { hop_set_err(parent, HOP_ERR_DEVICE, "hop_ctx_create_view_on: %s", hipGetErrorString(e)); hop_ctx_destroy(c); return HOP_ERR_DEVICE; }
  *out = c;
  return HOP_OK;
}

extern "C" {

const char* hop_version(void) { return "hophip 0.1 gfx950"; }
const char* hop_last_error(const hop_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

int hop_ctx_create(hop_ctx** out, int pic_w, int pic_h, int bit_depth_y, int bit_depth_c, int device) {
  if (!out) return hop_set_err(nullptr, HOP_ERR_ARG, "out is NULL");
  *out = nullptr;
  // picture sizes: the reference codes multiples of the minimum CU (8) only (TAppEncCfg padding)
  if (pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7)) return hop_set_err(nullptr, HOP_ERR_ARG, "picture %dx%d must be a positive multiple of 8", pic_w, pic_h);
  if (bit_depth_y < 8 || bit_depth_y > 12 || bit_depth_c < 8 || bit_depth_c > 12) return hop_set_err(nullptr, HOP_ERR_ARG, "bit depth out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return hop_set_err(nullptr, HOP_ERR_DEVICE, "no HIP device: libhophip has no CPU path");
  if (device < 0 || device >= ndev) return hop_set_err(nullptr, HOP_ERR_ARG, "device %d of %d", device, ndev);
  hop_ctx* c = (hop_ctx*)calloc(1, sizeof(hop_ctx));
  c->pic_w = pic_w; c->pic_h = pic_h; c->bd_y = bit_depth_y; c->bd_c = bit_depth_c; c->device = device;
  c->stride_y = pic_w + 2 * HOP_MARGIN_Y; c->stride_c = (pic_w >> 1) + 2 * HOP_MARGIN_C;
  c->pic_qps = (hop_pic_qps*)calloc(1, sizeof(hop_pic_qps));
  { const char* f = getenv("HOP_FUSED_LEAF"); c->fused_leaf_max = f ? atoi(f) : 8192; }
  { const char* f = getenv("HOP_WALK"); c->walk_max = f ? atoi(f) : 4096; }               // developer switch: the results do not depend on it
  { const char* f = getenv("HOP_SS_FAMILIES"); c->ss_families = !(f && f[0] == '0'); }   // developer switch: the results do not depend on it
  if (hipSetDevice(device) != hipSuccess) { free(c); return hop_set_err(nullptr, HOP_ERR_DEVICE, "hipSetDevice(%d) failed", device); }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    hop_set_err(nullptr, HOP_ERR_DEVICE, "device %d is '%s', libhophip is built for gfx950 only", device, prop.gcnArchName);
    free(c); return HOP_ERR_DEVICE;
  }
  size_t ny = (size_t)pic_w * pic_h, nc = ny >> 2;
  size_t sy = (size_t)c->stride_y * (pic_h + 2 * HOP_MARGIN_Y), sc = (size_t)c->stride_c * ((pic_h >> 1) + 2 * HOP_MARGIN_C);
  hipError_t e = create_lanes(c, hipStreamDefault, true);
  { const char* f = getenv("HOP_LANES"); c->lanes = f ? atoi(f) : 2; if (c->lanes < 1) c->lanes = 1; if (c->lanes > HOP_MAX_LANES) c->lanes = HOP_MAX_LANES; }
  if (e == hipSuccess) e = hipMalloc((void**)&c->org_y, ny * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->org_cb, nc * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->org_cr, nc * 2);
  const size_t gy = (size_t)HOP_GUARD_ROWS * c->stride_y, gc = (size_t)HOP_GUARD_ROWS * c->stride_c;
  if (e == hipSuccess) e = hipMalloc((void**)&c->ss_alloc[0], (sy + 2 * gy) * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->ss_alloc[1], (sc + 2 * gc) * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->ss_alloc[2], (sc + 2 * gc) * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->pred[0], ny * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->pred[1], nc * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->pred[2], nc * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->rec[0], ny * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->rec[1], nc * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->rec[2], nc * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&c->entropy_bits, 128 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(c->entropy_bits, hop_entropy_bits_host(), 128 * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&c->rdoq_scans, HOP_RDOQ_SCAN_ENTRIES * sizeof(uint16_t));
  if (e == hipSuccess) {
    std::vector<uint16_t> tabs(HOP_RDOQ_SCAN_ENTRIES);
    hop_rdoq_build_scans(tabs.data());
    e = hipMemcpy(c->rdoq_scans, tabs.data(), tabs.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) { hop_set_err(nullptr, HOP_ERR_DEVICE, "allocation failed: %s", hipGetErrorString(e)); hop_ctx_destroy(c); return HOP_ERR_DEVICE; }
  c->ss_buf[0] = c->ss_alloc[0] + gy; c->ss_buf[1] = c->ss_alloc[1] + gc; c->ss_buf[2] = c->ss_alloc[2] + gc;
  c->ss00[0] = c->ss_buf[0] + (size_t)HOP_MARGIN_Y * c->stride_y + HOP_MARGIN_Y;
  c->ss00[1] = c->ss_buf[1] + (size_t)HOP_MARGIN_C * c->stride_c + HOP_MARGIN_C;
  c->ss00[2] = c->ss_buf[2] + (size_t)HOP_MARGIN_C * c->stride_c + HOP_MARGIN_C;
  *out = c;
  int r = hop_ssref_reset(c);
  if (r == HOP_OK) r = hop_sync(c);
  if (r != HOP_OK) { strncpy(g_create_err, c->err, 511); hop_ctx_destroy(c); *out = nullptr; }
  return r;
}

// A second handle on the same pictures with its own stream and work areas: requests issued through different views run concurrently on the device.  The caller keeps
// their rectangles apart (the RD spine's CTU rows are a wavefront lag apart) and destroys the views before the parent.
int hop_ctx_create_view(hop_ctx* parent, hop_ctx** out) { return hop_ctx_create_view_on(parent, nullptr, out); }

// Several independent pictures of equal size in one context, so that one batch of requests serves CTUs of all of them (hop_encode_frame codes them side by side): the
// context's picture is their stack, picture k at rows k * sub_pitch .. k * sub_pitch + sub_h - 1, the rows between them unused.  The gap keeps every sample a picture's
// searches, margins and prefetches can touch (its margin + guard rows above and below) away from its neighbours', so each picture is coded exactly as in a context of its own.
// Candidate slots: the original, prediction and reconstruction pictures are laid out slots + 1 times one below the other (copy k at rows k * pic_h; the original is the
// same in all of them).  A request whose y coordinate is y + k * pic_h then works on copy k: candidates of one CU evaluated side by side predict, transform and
// reconstruct in copies of their own while searching the one SS reference (the predictor kernel takes the copy as hop_pred_job.dst_row_off).  Call before hop_upload_orig.
int hop_ctx_set_slots(hop_ctx* c, int slots) {
  if (!c || c->is_view || slots < 0 || slots > 128) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_slots: bad argument");
  if (slots == c->slots) return HOP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t ny = (size_t)c->pic_w * c->pic_h * (slots + 1), nc = ny >> 2;
  int16_t** planes[9] = { &c->org_y, &c->org_cb, &c->org_cr, &c->pred[0], &c->pred[1], &c->pred[2], &c->rec[0], &c->rec[1], &c->rec[2] };
  for (int k = 0; k < 9; k++) {
    if (*planes[k]) (void)hipFree(*planes[k]);
    *planes[k] = nullptr;
    hipError_t e = hipMalloc((void**)planes[k], ((k % 3) ? nc : ny) * 2);
    if (e != hipSuccess) return hop_set_err(c, HOP_ERR_DEVICE, "hop_ctx_set_slots: %s", hipGetErrorString(e));
  }
  c->slots = slots; c->have_orig = false;
  return HOP_OK;
}

int hop_set_fused_leaf(hop_ctx* c, int max_tus) { if (!c || max_tus < 0) return hop_set_err(c, HOP_ERR_ARG, "hop_set_fused_leaf: bad argument"); c->fused_leaf_max = max_tus; return HOP_OK; }

// Raster-order visibility for the searches of a wavefront: while on, every read of the SS reference by hop_me_search, hop_pred_inter / hop_pred_cost
// and hop_valid_pattern (and their *_device forms) finds the sentinel from the bottom of the CTU row that holds the PU's top-left sample on (hop_row_limit, hop_dev.h) --
// what the reference, which has coded nothing below the current CTU row, finds there.  The resident samples are not touched; hop_decode_frame ignores the switch.
int hop_ctx_set_row_limit(hop_ctx* c, int on) {
  if (!c) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_row_limit: bad argument");
  c->row_limit = on ? 1 : 0;
  return HOP_OK;
}

static void clear_picture_qps(hop_ctx* c) { if (c->pic_qps) { free(c->pic_qps->qp); c->pic_qps->qp = nullptr; c->pic_qps->n = 0; } }
int hop_stack_pitch(int sub_h) { return ((sub_h + 63) / 64) * 64 + 64 * ((2 * (HOP_MARGIN_Y + HOP_GUARD_ROWS) + 63) / 64); }
int hop_ctx_set_stack(hop_ctx* c, int sub_h, int sub_pitch) {
  if (!c || c->is_view) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_stack: bad argument");
  if (sub_h == 0 && sub_pitch == 0) { c->sub_h = c->sub_pitch = 0; clear_picture_qps(c); return HOP_OK; }
  if (sub_h <= 0 || (sub_h & 7) || (sub_pitch & 63) || sub_pitch < hop_stack_pitch(sub_h) || c->pic_h < sub_h || (c->pic_h - sub_h) % sub_pitch)
    return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_stack: a %d-row context is not a stack of %d-row pictures %d rows apart (pitch: a multiple of 64, at least hop_stack_pitch)", c->pic_h, sub_h, sub_pitch);
  c->sub_h = sub_h; c->sub_pitch = sub_pitch;
  clear_picture_qps(c);                                                 // the picture count changes
  return HOP_OK;
}

// One QP per picture of the context (include/hophip.h).  The table is the parent's; views read it through the pointer they copied (hop_picture_qps, hop_dev.h).
int hop_ctx_set_picture_qps(hop_ctx* c, int32_t n, const int32_t* qp) {
  if (!c || c->is_view || !c->pic_qps) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_picture_qps: bad argument (a view reads its parent's table)");
  if (n == 0 && !qp) { clear_picture_qps(c); return HOP_OK; }
  const int n_pic = hop_pictures(c, nullptr);
  if (n != n_pic || !qp) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_picture_qps: %d QPs%s, the context holds %d picture%s", n, qp ? "" : " (NULL)", n_pic, n_pic > 1 ? "s" : "");
  for (int k = 0; k < n; k++) if (qp[k] < 0 || qp[k] > 51) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_picture_qps: picture %d: qp %d is outside 0..51", k, qp[k]);
  int32_t* t = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
  if (!t) return hop_set_err(c, HOP_ERR_STATE, "hop_ctx_set_picture_qps: out of memory");
  memcpy(t, qp, sizeof(int32_t) * (size_t)n);
  free(c->pic_qps->qp); c->pic_qps->qp = t; c->pic_qps->n = n;
  return HOP_OK;
}

// The quantiser of the leaf step (include/hophip.h).  The word lives in the parent's shared object beside the QP table: views read it through the pointer they copied, and
// hop_make_pics hands it to every kernel that runs the leaf step (hop_pics::quant_mode).
int hop_ctx_set_quant_mode(hop_ctx* c, const hop_quant_mode* m) {
  if (!c || c->is_view || !c->pic_qps) return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_quant_mode: bad argument (a view reads its parent's mode)");
  if (!m) { c->pic_qps->quant_mode = 0; return HOP_OK; }
  if ((m->rdoq != 0 && m->rdoq != 1) || (m->rdoq_ts != 0 && m->rdoq_ts != 1))
    return hop_set_err(c, HOP_ERR_ARG, "hop_ctx_set_quant_mode: rdoq %d, rdoq_ts %d: each is 0 or 1", m->rdoq, m->rdoq_ts);
  c->pic_qps->quant_mode = (m->rdoq ? 0 : HOP_QM_FLAT) | (m->rdoq_ts ? 0 : HOP_QM_FLAT_TS) | (m->i_slice ? HOP_QM_I_SLICE : 0);
  return HOP_OK;
}

void hop_ctx_destroy(hop_ctx* c) {
  if (!c) return;
  if (c->stream) { (void)hipStreamSynchronize(c->stream); }
  if (c->is_view) {                                                     // pictures, tables and stash are the parent's
    c->org_y = c->org_cb = c->org_cr = nullptr; c->entropy_bits = nullptr; c->rdoq_scans = nullptr; c->stash = nullptr; c->coefpic = nullptr; c->coef_stash = nullptr;
    for (int k = 0; k < 3; k++) { c->ss_alloc[k] = nullptr; c->pred[k] = nullptr; c->rec[k] = nullptr; }
  }
  for (int i = 0; i < c->prof_cap; i++) { if (c->prof_recs[i].a) (void)hipEventDestroy(c->prof_recs[i].a); if (c->prof_recs[i].b) (void)hipEventDestroy(c->prof_recs[i].b); }
  free(c->prof_recs); free(c->rd_fraction);
  if (c->pic_qps && !c->is_view) { free(c->pic_qps->qp); free(c->pic_qps); }
  void* ptrs[] = { c->org_y, c->org_cb, c->org_cr, c->ss_alloc[0], c->ss_alloc[1], c->ss_alloc[2], c->pred[0], c->pred[1], c->pred[2],
                   c->rec[0], c->rec[1], c->rec[2], c->scratch, c->stage, c->rqt_buf, c->walk_buf, c->rdoq_scans, c->entropy_bits, c->stash, c->coefpic, c->coef_stash };
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (c->stream && !c->borrowed_stream) (void)hipStreamDestroy(c->stream);
  for (int k = 0; k < HOP_MAX_LANES - 1; k++) {
    const hop_lane& x = c->xlane[k];
    if (x.stream) (void)hipStreamDestroy(x.stream);
    if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]);
    for (void* p : { x.scratch, x.rqt_buf, x.walk_buf }) if (p) (void)hipFree(p);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  free(c);
}

int hop_sync(hop_ctx* c) { if (!c) return HOP_ERR_ARG; HIPCHK(c, hipStreamSynchronize(c->stream)); return HOP_OK; }
void* hop_stream(hop_ctx* c) { return c ? (void*)c->stream : nullptr; }

int hop_upload_orig(hop_ctx* c, const int16_t* y, int stride_y, const int16_t* cb, const int16_t* cr, int stride_c) {
  if (!c || !y || !cb || !cr || stride_y < c->pic_w || stride_c < (c->pic_w >> 1)) return hop_set_err(c, HOP_ERR_ARG, "hop_upload_orig: bad argument");
  HIPCHK(c, hipMemcpy2DAsync(c->org_y, (size_t)c->pic_w * 2, y, (size_t)stride_y * 2, (size_t)c->pic_w * 2, c->pic_h, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(c->org_cb, (size_t)c->pic_w, cb, (size_t)stride_c * 2, (size_t)c->pic_w, c->pic_h >> 1, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(c->org_cr, (size_t)c->pic_w, cr, (size_t)stride_c * 2, (size_t)c->pic_w, c->pic_h >> 1, hipMemcpyHostToDevice, c->stream));
  for (int k = 1; k <= c->slots; k++) {                                  // the copies of the candidate slots
    const size_t ny = (size_t)c->pic_w * c->pic_h, nc = ny >> 2;
    HIPCHK(c, hipMemcpyAsync(c->org_y + k * ny, c->org_y, ny * 2, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->org_cb + k * nc, c->org_cb, nc * 2, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->org_cr + k * nc, c->org_cr, nc * 2, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_orig = true;
  return HOP_OK;
}

int hop_ssref_reset(hop_ctx* c) { if (!c) return HOP_ERR_ARG; return hop_launch_ssref_reset(c); }

static size_t plane_elems(const hop_ctx* c, int comp) {
  return comp == 0 ? (size_t)c->stride_y * (c->pic_h + 2 * HOP_MARGIN_Y) : (size_t)c->stride_c * ((c->pic_h >> 1) + 2 * HOP_MARGIN_C);
}
int hop_ssref_download(hop_ctx* c, int comp, int16_t* dst) {
  if (!c || !dst || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_ssref_download: bad argument");
  HIPCHK(c, hipMemcpyAsync(dst, c->ss_buf[comp], plane_elems(c, comp) * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}
int hop_ssref_upload(hop_ctx* c, int comp, const int16_t* src) {
  if (!c || !src || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_ssref_upload: bad argument");
  HIPCHK(c, hipMemcpyAsync(c->ss_buf[comp], src, plane_elems(c, comp) * 2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}
int hop_pred_download(hop_ctx* c, int comp, int16_t* dst) {
  if (!c || !dst || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_pred_download: bad argument");
  size_t n = comp == 0 ? (size_t)c->pic_w * c->pic_h : ((size_t)c->pic_w * c->pic_h) >> 2;
  HIPCHK(c, hipMemcpyAsync(dst, c->pred[comp], n * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}

static int check_rects(hop_ctx* c, int n, const int32_t* r) {
  for (int i = 0; i < n; i++) {
    int x = r[4 * i], y = r[4 * i + 1], s = r[4 * i + 2];
    if (!(s == 8 || s == 16 || s == 32 || s == 64) || x < 0 || y < 0 || (x % s) || (y % s) || x + s > c->pic_w || y + s > c->pic_h)
      return hop_set_err(c, HOP_ERR_ARG, "hop_ssref_commit_cus: CU %d (%d,%d,%d) is not a legal CU of a %dx%d picture", i, x, y, s, c->pic_w, c->pic_h);
  }
  return HOP_OK;
}

int hop_ssref_commit_cus(hop_ctx* c, int n, const int32_t* rect4, const int16_t* rec_y, const int16_t* rec_cb, const int16_t* rec_cr) {
  if (!c || n < 0 || (n && (!rect4 || !rec_y || !rec_cb || !rec_cr))) return hop_set_err(c, HOP_ERR_ARG, "hop_ssref_commit_cus: bad argument");
  if (n == 0) return HOP_OK;
  int r = check_rects(c, n, rect4); if (r) return r;
  // packed layout: CU i's luma block starts at sum_{k<i} size_k^2; rect4[4*i+3] receives that offset
  std::vector<int32_t> rr(rect4, rect4 + 4 * (size_t)n);
  size_t tot = 0;
  for (int i = 0; i < n; i++) { rr[4 * i + 3] = (int32_t)tot; tot += (size_t)rr[4 * i + 2] * rr[4 * i + 2]; }
  stage_arena a(c);
  auto dr = a.in(rr.data(), rr.size()); auto dy = a.in(rec_y, tot); auto dcb = a.in(rec_cb, tot >> 2); auto dcr = a.in(rec_cr, tot >> 2);
  r = a.commit(0); if (r) return r;
  r = hop_launch_ssref_commit(c, n, a[dr], a[dy], a[dcb], a[dcr], 1); if (r) return r;
  return a.sync();
}

int hop_ssref_commit_cus_device(hop_ctx* c, int n, const int32_t* d_rect4, const int16_t* d_rec_y, const int16_t* d_rec_cb, const int16_t* d_rec_cr) {
  if (!c || n < 0 || (n && (!d_rect4 || !d_rec_y || !d_rec_cb || !d_rec_cr))) return hop_set_err(c, HOP_ERR_ARG, "hop_ssref_commit_cus_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_ssref_commit(c, n, d_rect4, d_rec_y, d_rec_cb, d_rec_cr, 0);
}

// host logic (hop_set_search_range, hop_component_bits, hop_bits_gt, hop_me_finish, the CABAC bin helpers): host/hop_hostlogic.cpp

// ---------------------------------------------------------------------------------------------
// hot path entry points
// ---------------------------------------------------------------------------------------------
static const int kLegalDim[] = { 4, 8, 12, 16, 24, 32, 48, 64 };
static bool legal_dim(int v) { for (int d : kLegalDim) if (v == d) return true; return false; }

}  // extern "C"
int hop_check_pu_jobs(hop_ctx* c, int n, const hop_pu_job* jobs) {
  for (int i = 0; i < n; i++) {
    const hop_pu_job& j = jobs[i];
    if (!legal_dim(j.w) || !legal_dim(j.h) || j.pu_x < 0 || j.pu_y < 0 || (j.pu_x & 3) || (j.pu_y & 3) || j.pu_x + j.w > c->pic_w || j.pu_y + j.h > c->pic_h)
      return hop_set_err(c, HOP_ERR_ARG, "PU job %d: rectangle (%d,%d,%dx%d) is not a legal PU of a %dx%d picture", i, j.pu_x, j.pu_y, j.w, j.h, c->pic_w, c->pic_h);
    if (j.n_amvp < 0 || j.n_amvp > 2) return hop_set_err(c, HOP_ERR_ARG, "PU job %d: n_amvp %d", i, j.n_amvp);
    // Reach: the reference addresses the padded plane linearly, so a column overshoot wraps into the neighbouring
    // row exactly as it does in the reference; what must hold is that every access stays inside the allocation:
    // rows (window, block, +4 probes, GT patch H/2 + 8-tap reach) within the 80-row margin, columns within one pitch.
    if (j.rng_right >= j.rng_left && j.rng_bottom >= j.rng_top) {
      if (j.rng_right - j.rng_left > 256 || j.rng_bottom - j.rng_top > 256)
        return hop_set_err(c, HOP_ERR_ARG, "PU job %d: search window larger than 257x257 (SearchRange > 128)", i);
      const int lim = HOP_MARGIN_Y + HOP_GUARD_ROWS - 4;
      bool bad = j.pu_y + j.rng_top - j.h / 2 - 4 < -lim || j.pu_y + j.rng_bottom + j.h + j.h / 2 + 8 > c->pic_h + lim ||
                 j.pu_x + j.rng_left - j.w / 2 - 4 < -(c->stride_y - 8) || j.pu_x + j.rng_right + 2 * j.w + 8 > c->stride_y + c->pic_w - 8;
      for (int k = 0; k < j.n_amvp; k++) {   // AMVP start vectors of the GT search (TEncSearch.cpp:5144-5150)
        const int sx = (int)(int16_t)j.amvp[2 * k] >> 2, sy = (int)(int16_t)j.amvp[2 * k + 1] >> 2;
        bad = bad || j.pu_y + sy - j.h / 2 < -lim || j.pu_y + sy + j.h + j.h / 2 > c->pic_h + lim ||
              j.pu_x + sx - j.w / 2 - 4 < -(c->stride_y - 8) || j.pu_x + sx + 2 * j.w + 8 > c->stride_y + c->pic_w - 8;   // columns: within one pitch, as for the window (a neighbour's unclipped vector may point past the margin)
      }
      if (bad)
        return hop_set_err(c, HOP_ERR_ARG, "PU job %d: search range leaves the padded reference", i);
    }
  }
  return HOP_OK;
}
extern "C" {

static int me_pipeline(hop_ctx* c, int n, const hop_pu_job* d_jobs, hop_pu_result* d_results, int stage) {
  int r = hop_launch_ss_search(c, n, d_jobs, d_results); if (r) return r;
  if (stage >= HOP_STAGE_FRAC) { r = hop_launch_frac(c, n, d_jobs, d_results); if (r) return r; }
  if (stage >= HOP_STAGE_GT) { r = hop_launch_gt(c, n, d_jobs, d_results); if (r) return r; }
  return HOP_OK;
}

int hop_set_lanes(hop_ctx* c, int lanes) {
  if (!c || lanes < 1 || lanes > HOP_MAX_LANES) return hop_set_err(c, HOP_ERR_ARG, "hop_set_lanes: 1..%d", HOP_MAX_LANES);
  c->lanes = lanes;
  return HOP_OK;
}

int hop_me_search_device(hop_ctx* c, int n, const hop_pu_job* d_jobs, hop_pu_result* d_results, int stage) {
  if (!c || n < 0 || stage < HOP_STAGE_INT || stage > HOP_STAGE_GT || (n && (!d_jobs || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_me_search_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_me_search: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  // Large batches are cut into parts (at multiples of 5 PUs, so that a list of whole CUs keeps its families) that run on
  // separate streams: PUs are independent, the results do not depend on the cut.
  const int parts = (n >= 16384) ? c->lanes : 1;
  const int per = ((n + parts - 1) / parts + 4) / 5 * 5;
  return run_on_lanes(c, parts, "hop_me_search_device", [&](int k) {
    const int o = k * per, m = std::min(per, n - o);
    return m > 0 ? me_pipeline(c, m, d_jobs + o, d_results + o, stage) : HOP_OK;
  });
}

int hop_me_search(hop_ctx* c, int n, const hop_pu_job* jobs, hop_pu_result* results, int stage) {
  if (!c || n < 0 || (n && (!jobs || !results))) return hop_set_err(c, HOP_ERR_ARG, "hop_me_search: bad argument");
  if (n == 0) return HOP_OK;
  int r = hop_check_pu_jobs(c, n, jobs); if (r) return r;
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dr = a.out<hop_pu_result>(n);
  r = a.commit(0); if (r) return r;
  r = hop_me_search_device(c, n, a[dj], a[dr], stage); if (r) return r;
  r = a.download(results, dr); if (r) return r;
  return a.sync();
}

int hop_pred_inter_device(hop_ctx* c, int n, const hop_pred_job* d_jobs) {
  if (!c || n < 0 || (n && !d_jobs)) return hop_set_err(c, HOP_ERR_ARG, "hop_pred_inter_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_pred(c, n, d_jobs);
}

__global__ void k_gather_pred(const hop_pred_job* jobs, const int64_t* offs, const int16_t* py, const int16_t* pcb, const int16_t* pcr,
                              int pic_w, int16_t* oy, int16_t* ocb, int16_t* ocr) {
  hop_pred_job j = jobs[blockIdx.x];
  int64_t o = offs[blockIdx.x];
  for (int i = threadIdx.x; i < j.w * j.h; i += blockDim.x) {
    int r = i / j.w, cc = i % j.w;
    oy[o + i] = py[(size_t)(j.pu_y + r) * pic_w + j.pu_x + cc];
  }
  int cw = j.w >> 1, ch = j.h >> 1;
  for (int i = threadIdx.x; i < cw * ch; i += blockDim.x) {
    int r = i / cw, cc = i % cw;
    size_t s = (size_t)((j.pu_y >> 1) + r) * (pic_w >> 1) + (j.pu_x >> 1) + cc;
    ocb[(o >> 2) + i] = pcb[s]; ocr[(o >> 2) + i] = pcr[s];
  }
}

}  // extern "C"
// what every predictor job must satisfy before a kernel may run on it (shapes, candidate slot, the reach of the doubled patch + 8-tap filter inside the padded reference)
int hop_check_pred_jobs(hop_ctx* c, int n, const hop_pred_job* jobs) {
  for (int i = 0; i < n; i++) {
    const hop_pred_job& j = jobs[i];
    if (!legal_dim(j.w) || !legal_dim(j.h) || j.pu_x < 0 || j.pu_y < 0 || (j.pu_x & 3) || (j.pu_y & 3) || j.pu_x + j.w > c->pic_w || j.pu_y + j.h > c->pic_h)
      return hop_set_err(c, HOP_ERR_ARG, "pred job %d: illegal PU rectangle", i);
    if (j.dst_row_off < 0 || j.dst_row_off % c->pic_h || j.dst_row_off / c->pic_h > c->slots) return hop_set_err(c, HOP_ERR_ARG, "pred job %d: dst_row_off %d is not one of the context's %d candidate slots", i, j.dst_row_off, c->slots);
    // reach of the doubled patch + 8-tap filter must stay in the margin
    int ix = j.pu_x + (j.mv_x >> 2), iy = j.pu_y + (j.mv_y >> 2);
    const int lim = HOP_MARGIN_Y + HOP_GUARD_ROWS - 4;      // rows may use the guard band, columns wrap linearly like the reference
    if (iy - j.h / 2 - 4 < -lim || iy + j.h + j.h / 2 + 4 >= c->pic_h + lim || ix - j.w / 2 - 4 < -(c->stride_y - 8) || ix + 2 * j.w + 8 > c->stride_y + c->pic_w - 8)
      return hop_set_err(c, HOP_ERR_ARG, "pred job %d: motion vector leaves the padded reference", i);
  }
  return HOP_OK;
}
extern "C" {

int hop_pred_inter(hop_ctx* c, int n, const hop_pred_job* jobs, int16_t* out_y, int16_t* out_cb, int16_t* out_cr) {
  if (!c || n < 0 || (n && !jobs)) return hop_set_err(c, HOP_ERR_ARG, "hop_pred_inter: bad argument");
  if (n == 0) return HOP_OK;
  { int rc = hop_check_pred_jobs(c, n, jobs); if (rc) return rc; }
  std::vector<int64_t> offs(n);
  size_t tot = 0;
  for (int i = 0; i < n; i++) { offs[i] = (int64_t)tot; tot += (size_t)jobs[i].w * jobs[i].h; }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto d_off = a.out<int64_t>(n); auto dy = a.out<int16_t>(tot); auto dcb = a.out<int16_t>(tot / 4); auto dcr = a.out<int16_t>(tot / 4);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_pred(c, n, a[dj]); if (r) return r;
  if (out_y && out_cb && out_cr) {
    r = a.upload(d_off, offs.data()); if (r) return r;
    hipLaunchKernelGGL(k_gather_pred, dim3(n), dim3(256), 0, c->stream, (const hop_pred_job*)a[dj], (const int64_t*)a[d_off],
                       c->pred[0], c->pred[1], c->pred[2], c->pic_w, a[dy], a[dcb], a[dcr]);
    HIPCHK(c, hipGetLastError());
    if ((r = a.download(out_y, dy)) || (r = a.download(out_cb, dcb)) || (r = a.download(out_cr, dcr))) return r;
  }
  return a.sync();
}

int hop_pred_upload(hop_ctx* c, int comp, const int16_t* src) {
  if (!c || !src || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_pred_upload: bad argument");
  size_t n = comp == 0 ? (size_t)c->pic_w * c->pic_h : ((size_t)c->pic_w * c->pic_h) >> 2;
  HIPCHK(c, hipMemcpyAsync(c->pred[comp], src, n * 2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}
int hop_recon_upload(hop_ctx* c, int comp, const int16_t* src) {
  if (!c || !src || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_recon_upload: bad argument");
  size_t n = comp == 0 ? (size_t)c->pic_w * c->pic_h : ((size_t)c->pic_w * c->pic_h) >> 2;
  HIPCHK(c, hipMemcpyAsync(c->rec[comp], src, n * 2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}
int hop_recon_download(hop_ctx* c, int comp, int16_t* dst) {
  if (!c || !dst || comp < 0 || comp > 2) return hop_set_err(c, HOP_ERR_ARG, "hop_recon_download: bad argument");
  size_t n = comp == 0 ? (size_t)c->pic_w * c->pic_h : ((size_t)c->pic_w * c->pic_h) >> 2;
  HIPCHK(c, hipMemcpyAsync(dst, c->rec[comp], n * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}

int hop_tu_roundtrip(hop_ctx* c, int n, const hop_tu_job* jobs, hop_tu_result* results, int32_t* levels_out) {
  if (!c || n < 0 || (n && (!jobs || !results))) return hop_set_err(c, HOP_ERR_ARG, "hop_tu_roundtrip: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_tu_roundtrip: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<int64_t> offs(n);
  size_t tot = 0;
  for (int i = 0; i < n; i++) {
    const hop_tu_job& j = jobs[i];
    const int N = 1 << j.log2_size, sh = j.comp ? 1 : 0;
    if (j.comp < 0 || j.comp > 2 || j.log2_size < 2 || j.log2_size > 5 || j.x < 0 || j.y < 0 || ((j.x >> sh) & 3) || ((j.y >> sh) & 3) ||
        (j.x >> sh) + N > (c->pic_w >> sh) || (j.y >> sh) + N > (c->pic_h >> sh) || j.qp_scaled < 0 || j.qp_scaled > 87 || (j.use_dst && (j.log2_size != 2 || j.comp != 0)) || j.scan_idx < 0 || j.scan_idx > 2)
      return hop_set_err(c, HOP_ERR_ARG, "TU job %d: illegal transform unit", i);
    offs[i] = (int64_t)tot; tot += (size_t)N * N;
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dr = a.out<hop_tu_result>(n); auto d_off = a.in(offs.data(), n); auto dl = a.out<int32_t>(levels_out ? tot : 0);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_tu(c, n, a[dj], a[dr], levels_out ? a[dl] : nullptr, a[d_off]); if (r) return r;
  r = a.download(results, dr); if (r) return r;
  if (levels_out && (r = a.download(levels_out, dl))) return r;
  return a.sync();
}

int hop_intra_rough(hop_ctx* c, int n, const hop_intra_job* jobs, uint32_t* satd_out) {
  if (!c || n < 0 || (n && (!jobs || !satd_out))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_rough: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_rough: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  int u = 0;
  for (int i = 0; i < n; i++) {
    if (!intra_block_ok(c, jobs[i], 0)) return hop_set_err(c, HOP_ERR_ARG, "intra job %d: illegal block", i);
    if (!intra_neighbours_ok(c, jobs[i], 0, &u)) return hop_set_err(c, HOP_ERR_ARG, "intra job %d: neighbour unit %d flagged available but outside the picture", i, u);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto ds = a.out<uint32_t>((size_t)n * 35);
  int r = a.commit(0); if (r) return r;
  r = hop_launch_intra(c, n, a[dj], a[ds]); if (r) return r;
  r = a.download(satd_out, ds); if (r) return r;
  return a.sync();
}

int hop_tu_roundtrip_device(hop_ctx* c, int n, const hop_tu_job* d_jobs, hop_tu_result* d_results, int32_t* d_levels, const int64_t* d_level_offsets) {
  if (!c || n < 0 || (n && (!d_jobs || !d_results)) || (d_levels && !d_level_offsets)) return hop_set_err(c, HOP_ERR_ARG, "hop_tu_roundtrip_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_tu_roundtrip: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  return hop_launch_tu(c, n, d_jobs, d_results, d_levels, d_level_offsets);
}

int hop_intra_rough_device(hop_ctx* c, int n, const hop_intra_job* d_jobs, uint32_t* d_satd) {
  if (!c || n < 0 || (n && (!d_jobs || !d_satd))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_rough_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_rough: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  return hop_launch_intra(c, n, d_jobs, d_satd);
}

int hop_rdoq_device(hop_ctx* c, int n, const hop_rdoq_job* d_jobs, const hop_estbits* d_tables, const int32_t* d_src, int32_t* d_dst, uint32_t* d_abs_sum) {
  if (!c || n < 0 || (n && (!d_jobs || !d_tables || !d_src || !d_dst || !d_abs_sum))) return hop_set_err(c, HOP_ERR_ARG, "hop_rdoq_device: bad argument");
  if (n == 0) return HOP_OK;
  void* work; int r = hop_scratch(c, hop_rdoq_work_bytes(n), &work); if (r) return r;
  return hop_launch_rdoq(c, n, d_jobs, d_tables, d_src, d_dst, d_abs_sum, work);
}

int hop_rdoq(hop_ctx* c, int n, const hop_rdoq_job* jobs, int n_tables, const hop_estbits* tables, size_t n_coeff,
             const int32_t* src, int32_t* dst, uint32_t* abs_sum) {
  if (!c || n < 0 || (n && (!jobs || !tables || !src || !dst || !abs_sum || n_tables <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_rdoq: bad argument");
  if (n == 0) return HOP_OK;
  for (int i = 0; i < n; i++) {
    const hop_rdoq_job& j = jobs[i];
    const size_t n2 = (size_t)1 << (2 * j.log2_size);
    if (j.log2_size < 2 || j.log2_size > 5 || j.comp < 0 || j.comp > 2 || (j.comp && j.log2_size == 5) || j.scan_idx < 0 || j.scan_idx > 2 ||
        j.tr_depth < 0 || j.tr_depth > 3 || j.qp_scaled < 0 || j.qp_scaled > 87 || j.bit_depth < 8 || j.bit_depth > 12 || !(j.lambda > 0.0) ||
        j.coeff_offset < 0 || (size_t)j.coeff_offset + n2 > n_coeff || j.estbits_index < 0 || j.estbits_index >= n_tables)
      return hop_set_err(c, HOP_ERR_ARG, "RDOQ job %d: illegal transform unit / table / offset", i);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dt = a.in(tables, n_tables); auto ds = a.in(src, n_coeff); auto dd = a.zero<int32_t>(n_coeff); auto da = a.out<uint32_t>(n);
  int r = a.commit(256); if (r) return r;
  void* work; r = hop_scratch(c, hop_rdoq_work_bytes(n), &work); if (r) return r;
  r = hop_launch_rdoq(c, n, a[dj], a[dt], a[ds], a[dd], a[da], work); if (r) return r;
  if ((r = a.download(dst, dd)) || (r = a.download(abs_sum, da))) return r;
  return a.sync();
}

int hop_coeff_bits_device(hop_ctx* c, int n, const hop_coeff_bits_job* d_jobs, const hop_cabac_ctx* d_ctx_in, const int32_t* d_coef,
                          uint64_t* d_bits, hop_cabac_ctx* d_ctx_out) {
  if (!c || n < 0 || (n && (!d_jobs || !d_ctx_in || !d_coef || !d_bits))) return hop_set_err(c, HOP_ERR_ARG, "hop_coeff_bits_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_coeff_bits(c, n, d_jobs, d_ctx_in, d_coef, (unsigned long long*)d_bits, d_ctx_out);
}

int hop_coeff_bits(hop_ctx* c, int n, const hop_coeff_bits_job* jobs, int n_ctx, const hop_cabac_ctx* ctx_in, size_t n_coeff,
                   const int32_t* coef, uint64_t* bits, hop_cabac_ctx* ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !ctx_in || !coef || !bits || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_coeff_bits: bad argument");
  if (n == 0) return HOP_OK;
  for (int i = 0; i < n; i++) {
    const hop_coeff_bits_job& j = jobs[i];
    if (j.log2_size < 2 || j.log2_size > 5 || j.comp < 0 || j.comp > 2 || (j.comp && j.log2_size == 5) || j.scan_idx < 0 || j.scan_idx > 2 ||
        j.ctx_index < 0 || j.ctx_index >= n_ctx || j.coeff_offset < 0 || (size_t)j.coeff_offset + ((size_t)1 << (2 * j.log2_size)) > n_coeff)
      return hop_set_err(c, HOP_ERR_ARG, "coeff-bits job %d: illegal transform unit / context index / offset", i);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, nullptr)) return HOP_ERR_ARG;
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dc = a.in(ctx_in, n_ctx); auto ds = a.in(coef, n_coeff); auto db = a.out<uint64_t>(n); auto dx = a.out<hop_cabac_ctx>(ctx_out ? n : 0);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_coeff_bits(c, n, a[dj], a[dc], a[ds], (unsigned long long*)a[db], ctx_out ? a[dx] : nullptr); if (r) return r;
  r = a.download(bits, db); if (r) return r;
  if (ctx_out && (r = a.download(ctx_out, dx))) return r;
  return a.sync();
}

int hop_tu_rd_device(hop_ctx* c, int n, const hop_tu_rd_job* d_jobs, const hop_cabac_ctx* d_ctx_in, const int64_t* d_coef_offsets, size_t n_coeff,
                     int32_t* d_levels, hop_tu_rd_result* d_results) {
  if (!c || n < 0 || (n && (!d_jobs || !d_ctx_in || !d_coef_offsets || !d_levels || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_tu_rd_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_tu_rd: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  return hop_launch_tu_rd(c, n, d_jobs, d_ctx_in, d_coef_offsets, n_coeff, d_levels, d_results, 0);
}

int hop_intra_modes_device(hop_ctx* c, int n, const hop_intra_modes_job* d_jobs, const uint32_t* d_satd, hop_intra_modes_result* d_results) {
  if (!c || n < 0 || (n && (!d_jobs || !d_satd || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_modes_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_intra_modes(c, n, d_jobs, d_satd, d_results);
}

int hop_intra_modes(hop_ctx* c, int n, const hop_intra_modes_job* jobs, const uint32_t* satd, hop_intra_modes_result* results) {
  if (!c || n < 0 || (n && (!jobs || !satd || !results))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_modes: bad argument");
  if (n == 0) return HOP_OK;
  for (int i = 0; i < n; i++) {
    const hop_intra_modes_job& j = jobs[i];
    bool ok = j.pred_num >= 0 && j.pred_num <= 3 && j.mpm_cand >= 0 && j.mpm_cand <= j.pred_num && j.num_full_rd >= 1 && j.num_full_rd <= 8 && j.ctx_state >= 0 && j.ctx_state <= 127 &&
              j.frac_left >= 0 && j.frac_left < 32768 && j.sqrt_lambda > 0.0;
    for (int k = 0; k < j.pred_num && ok; k++) ok = j.preds[k] >= 0 && j.preds[k] < 35;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra modes job %d: illegal predictors / list size / context", i);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto ds = a.in(satd, (size_t)n * 35); auto dr = a.out<hop_intra_modes_result>(n);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_intra_modes(c, n, a[dj], a[ds], a[dr]); if (r) return r;
  r = a.download(results, dr); if (r) return r;
  return a.sync();
}

int hop_rqt_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, const hop_cabac_ctx* d_ctx_in, hop_rqt_result* d_results, int32_t* d_coef_out,
                   hop_cabac_ctx* d_ctx_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_ctx_in || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_rqt: hop_upload_orig has not been called");
  if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_device: illegal CU class");
  if (n == 0) return HOP_OK;
  int r = rqt_reserve(c, hop_rqt_work_bytes(cls->log2_cu, n)); if (r) return r;
  return hop_launch_rqt_class(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->inter_split_flag ? 1 : 0, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, n, d_jobs,
                              d_ctx_in, d_results, d_coef_out, d_ctx_out, c->rqt_buf, c->rqt_bytes);
}

int hop_rqt_device_classes(hop_ctx* c, int n_classes, const int* n, const hop_rqt_job* const* d_jobs, const hop_rqt_job* cls, const hop_cabac_ctx* d_ctx_in,
                           hop_rqt_result* const* d_results, int32_t* const* d_coef_out, hop_cabac_ctx* const* d_ctx_out) {
  if (!c || n_classes < 0 || (n_classes && (!n || !d_jobs || !cls || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_device_classes: bad argument");
  if (n_classes == 0) return HOP_OK;
  // classes are independent chains of small kernels: each runs on its own stream (with its own scratch and state buffers)
  return run_on_lanes(c, n_classes, "hop_rqt_device_classes", [&](int i) {
    return hop_rqt_device(c, n[i], d_jobs[i], cls + i, d_ctx_in, d_results[i], d_coef_out ? d_coef_out[i] : nullptr, d_ctx_out ? d_ctx_out[i] : nullptr);
  });
}

int hop_rqt(hop_ctx* c, int n, const hop_rqt_job* jobs, int n_ctx, const hop_cabac_ctx* ctx_in, hop_rqt_result* results, int32_t* coef_out, hop_cabac_ctx* ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !ctx_in || !results || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_rqt: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i];
    bool ok = rqt_class_ok(j) && cu_rect_ok(c, j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0;
    for (int k = 0; k < 3 && ok; k++) ok = j.qp_scaled[k] >= 0 && j.qp_scaled[k] <= 87 && j.lambda_rdoq[k] > 0.0;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "RQT job %d: illegal CU / transform-tree limits / snapshot / parameters", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, nullptr)) return HOP_ERR_ARG;
  // one pass per class of CUs (same size and transform-tree limits): the walk over the tree is the same for all of them
  auto same = [&](int p, int q) { return same_tree(jobs[p], jobs[q]) && !jobs[p].inter_split_flag == !jobs[q].inter_split_flag && !jobs[p].sign_hide == !jobs[q].sign_hide; };
  return for_each_class(n, same, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx);
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dc = a.in(ctx_in, n_ctx); auto dr = a.out<hop_rqt_result>(m); auto d_co = a.out<int32_t>(m * cu3); auto dx = a.out<hop_cabac_ctx>(m);
    a.end_mark();
    int r = a.commit(256); if (r) return r;
    r = hop_rqt_device(c, (int)m, a[dj], &f, a[dc], a[dr], a[d_co], a[dx]); if (r) return r;
    std::vector<hop_rqt_result> rr(m); std::vector<int32_t> co(m * cu3); std::vector<hop_cabac_ctx> cx(m);
    if ((r = a.download(rr.data(), dr)) || (r = a.download(co.data(), d_co)) || (r = a.download(cx.data(), dx)) || (r = a.sync())) return r;
    scatter(results, idx, rr.data());
    if (coef_out) scatter(coef_out, idx, co.data(), cu3, coff.data());
    if (ctx_out) scatter(ctx_out, idx, cx.data());
    return (int)HOP_OK;
  });
}

int hop_rqt_finish_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, hop_rqt_result* d_results, int32_t* d_coef, const hop_cabac_ctx* d_ctx_after,
                          hop_cu_final* d_finals) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_results || !d_coef || !d_ctx_after || !d_finals))) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_finish_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_rqt_finish: hop_upload_orig has not been called");
  if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_finish_device: illegal CU class");
  if (n == 0) return HOP_OK;
  int r = rqt_reserve(c, hop_rqt_finish_work_bytes(cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, n)); if (r) return r;
  return hop_launch_rqt_finish(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->use_ts ? 1 : 0, n, d_jobs, d_results, d_coef, d_ctx_after, d_finals, c->rqt_buf);
}

int hop_rqt_finish(hop_ctx* c, int n, const hop_rqt_job* jobs, hop_rqt_result* results, int32_t* coef, const hop_cabac_ctx* ctx_after, hop_cu_final* finals) {
  if (!c || n < 0 || (n && (!jobs || !results || !coef || !ctx_after || !finals))) return hop_set_err(c, HOP_ERR_ARG, "hop_rqt_finish: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_rqt_finish: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i];
    if (!(rqt_class_ok(j) && cu_rect_ok(c, j) && j.lambda_rd > 0.0)) return hop_set_err(c, HOP_ERR_ARG, "RQT finish job %d: illegal CU / transform-tree limits / parameters", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  return for_each_class(n, [&](int p, int q) { return same_tree(jobs[p], jobs[q]); }, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_cabac_ctx> cx = gather(ctx_after, idx);
    std::vector<hop_rqt_result> rr = gather(results, idx); std::vector<int32_t> co = gather(coef, idx, cu3, coff.data());
    stage_arena a(c);                                                  // the kernel's work area is the tail of the same reservation
    auto dj = a.in(cls.data(), m); auto dr = a.in(rr.data(), m); auto d_co = a.in(co.data(), m * cu3); auto dx = a.in(cx.data(), m); auto df = a.out<hop_cu_final>(m);
    auto dw = a.out<char>(hop_rqt_finish_work_bytes(f.log2_cu, f.log2_max_tu, f.log2_min_tu_in_cu, (int)m));
    int r = a.commit(256); if (r) return r;
    r = hop_launch_rqt_finish(c, f.log2_cu, f.log2_max_tu, f.log2_min_tu_in_cu, f.use_ts ? 1 : 0, (int)m, a[dj], a[dr], a[d_co], a[dx], a[df], a[dw]); if (r) return r;
    std::vector<hop_cu_final> ff(m);
    if ((r = a.download(rr.data(), dr)) || (r = a.download(co.data(), d_co)) || (r = a.download(ff.data(), df)) || (r = a.sync())) return r;
    scatter(results, idx, rr.data()); scatter(finals, idx, ff.data()); scatter(coef, idx, co.data(), cu3, coff.data());
    return (int)HOP_OK;
  });
}

int hop_intra_cu_bits(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_intra_cu_syntax* syntax, const hop_rqt_result* results, const int32_t* coef, int n_ctx,
                      const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in, uint32_t* bits, hop_cabac_ctx* ctx_out, hop_cabac_cu_ctx* cu_ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !results || !coef || !ctx_in || !cu_ctx_in || !bits || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_bits: bad argument");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_intra_cu_syntax& y = syntax[i];
    const int parts = 1 << (2 * (j.log2_cu - 2));
    bool ok = rqt_class_ok(j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && y.skip_ctx >= 0 && y.skip_ctx <= 2 &&
              y.tr_depth >= 0 && y.tr_depth <= 3 && y.part >= 0 && y.part < parts && (y.part % (parts >> (2 * y.tr_depth))) == 0 && (y.b_luma || y.b_chroma);
    for (int p = 0; p < (y.part_nxn ? 4 : 1) && ok; p++) ok = y.luma_dir[p] >= 0 && y.luma_dir[p] < 35 && y.pred_num[p] >= 0 && y.pred_num[p] <= 3;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra CU bits job %d: illegal CU class / node / syntax elements / snapshot", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  return for_each_class(n, [&](int p, int q) { return same_tree(jobs[p], jobs[q]) && !jobs[p].sign_hide == !jobs[q].sign_hide; }, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_intra_cu_syntax> sy = gather(syntax, idx);
    const std::vector<hop_rqt_result> rr = gather(results, idx); const std::vector<int32_t> co = gather(coef, idx, cu3, coff.data());
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dr = a.in(rr.data(), m); auto d_co = a.in(co.data(), m * cu3); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
    auto db = a.out<uint32_t>(m); auto dx = a.out<hop_cabac_ctx>(m); auto dv = a.out<hop_cabac_cu_ctx>(m);
    a.end_mark();
    int r = a.commit(256); if (r) return r;
    r = hop_launch_intra_cu_bits(c, f.log2_cu, f.log2_max_tu, f.log2_min_tu_in_cu, f.sign_hide ? 1 : 0, f.use_ts ? 1 : 0, (int)m, a[dj], a[dy], a[dr], a[d_co], a[dc], a[du], a[db], a[dx], a[dv]);
    if (r) return r;
    std::vector<uint32_t> bb(m); std::vector<hop_cabac_ctx> cx(m); std::vector<hop_cabac_cu_ctx> cv(m);
    if ((r = a.download(bb.data(), db)) || (r = a.download(cx.data(), dx)) || (r = a.download(cv.data(), dv)) || (r = a.sync())) return r;
    scatter(bits, idx, bb.data());
    if (ctx_out) scatter(ctx_out, idx, cx.data());
    if (cu_ctx_out) scatter(cu_ctx_out, idx, cv.data());
    return (int)HOP_OK;
  });
}

int hop_intra_rqt_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, int tr_depth, int check_first, const hop_intra_cu_syntax* d_syntax,
                         const hop_intra_rqt_opt* d_opts, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in, hop_rqt_result* d_results, int32_t* d_coef_out,
                         hop_cabac_ctx* d_ctx_out, hop_cabac_cu_ctx* d_cu_ctx_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_syntax || !d_opts || !d_ctx_in || !d_cu_ctx_in || !d_results))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_rqt_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_rqt: hop_upload_orig has not been called");
  if (!rqt_class_ok(*cls) || tr_depth < 0 || tr_depth > 1 || cls->log2_cu - tr_depth < cls->log2_min_tu_in_cu)
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_rqt_device: illegal PU class");
  if (n == 0) return HOP_OK;
  int r = rqt_reserve(c, hop_intra_rqt_work_bytes(cls->log2_cu, n)); if (r) return r;
  return hop_launch_intra_rqt(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, tr_depth, check_first ? 1 : 0, n, d_jobs, d_syntax,
                              d_opts, d_ctx_in, d_cu_ctx_in, d_results, d_coef_out, d_ctx_out, d_cu_ctx_out, c->rqt_buf, c->rqt_bytes, nullptr);
}

int hop_intra_rqt(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_intra_cu_syntax* syntax, const hop_intra_rqt_opt* opts, int n_ctx, const hop_cabac_ctx* ctx_in,
                  const hop_cabac_cu_ctx* cu_ctx_in, hop_rqt_result* results, int32_t* coef_out, hop_cabac_ctx* ctx_out, hop_cabac_cu_ctx* cu_ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !opts || !ctx_in || !cu_ctx_in || !results || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_rqt: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_rqt: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_intra_cu_syntax& y = syntax[i];
    const int parts = 1 << (2 * (j.log2_cu - 2));
    bool ok = rqt_class_ok(j) && cu_rect_ok(c, j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0 && j.qp_scaled[0] >= 0 && j.qp_scaled[0] <= 87 && j.lambda_rdoq[0] > 0.0 &&
              y.skip_ctx >= 0 && y.skip_ctx <= 2 && (y.tr_depth == 0 || y.tr_depth == 1) && !y.part_nxn == !y.tr_depth && y.part >= 0 && y.part < parts &&
              (y.part % (parts >> (2 * y.tr_depth))) == 0 && j.log2_cu - y.tr_depth >= j.log2_min_tu_in_cu;
    for (int p = 0; p < (y.part_nxn ? 4 : 1) && ok; p++) ok = y.luma_dir[p] >= 0 && y.luma_dir[p] < 35 && y.pred_num[p] >= 0 && y.pred_num[p] <= 3;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra RQT job %d: illegal CU / PU node / transform-tree limits / syntax elements / snapshot / parameters", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  auto same = [&](int p, int q) {
    return same_tree(jobs[p], jobs[q]) && !jobs[p].sign_hide == !jobs[q].sign_hide && syntax[p].tr_depth == syntax[q].tr_depth && !opts[p].check_first == !opts[q].check_first;
  };
  return for_each_class(n, same, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]]; const int d0 = syntax[idx[0]].tr_depth, cf = opts[idx[0]].check_first ? 1 : 0;
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_intra_cu_syntax> sy = gather(syntax, idx); const std::vector<hop_intra_rqt_opt> op = gather(opts, idx);
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dp = a.in(op.data(), m); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
    auto dr = a.out<hop_rqt_result>(m); auto d_co = a.zero<int32_t>(m * cu3); auto dx = a.out<hop_cabac_ctx>(m); auto dv = a.out<hop_cabac_cu_ctx>(m);
    a.end_mark();
    int r = a.commit(256); if (r) return r;
    r = hop_intra_rqt_device(c, (int)m, a[dj], &f, d0, cf, a[dy], a[dp], a[dc], a[du], a[dr], a[d_co], a[dx], a[dv]); if (r) return r;
    std::vector<hop_rqt_result> rr(m); std::vector<int32_t> co(m * cu3); std::vector<hop_cabac_ctx> cx(m); std::vector<hop_cabac_cu_ctx> cv(m);
    if ((r = a.download(rr.data(), dr)) || (r = a.download(co.data(), d_co)) || (r = a.download(cx.data(), dx)) || (r = a.download(cv.data(), dv)) || (r = a.sync())) return r;
    scatter(results, idx, rr.data());
    if (coef_out) scatter(coef_out, idx, co.data(), cu3, coff.data());
    if (ctx_out) scatter(ctx_out, idx, cx.data());
    if (cu_ctx_out) scatter(cu_ctx_out, idx, cv.data());
    return (int)HOP_OK;
  });
}

int hop_intra_luma_search_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, int part_nxn, int num_full_rd, const hop_intra_cu_syntax* d_syntax,
                                 const hop_intra_rqt_opt* d_opts, const hop_intra_search_job* d_sjobs, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in,
                                 hop_intra_search_result* d_sresults, hop_rqt_result* d_results, int32_t* d_coef_out, int16_t* d_reco_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_syntax || !d_opts || !d_sjobs || !d_ctx_in || !d_cu_ctx_in || !d_sresults || !d_results || !d_coef_out || !d_reco_out)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_luma_search_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_luma_search: hop_upload_orig has not been called");
  const int nxn = part_nxn ? 1 : 0;
  if (!rqt_class_ok(*cls) || cls->log2_cu - nxn < cls->log2_min_tu_in_cu || num_full_rd < 1 || num_full_rd > 8)
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_luma_search_device: illegal CU class");
  if (n == 0) return HOP_OK;
  int r = rqt_reserve(c, hop_intra_search_work_bytes(cls->log2_cu, n)); if (r) return r;
  return hop_launch_intra_search(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, nxn, num_full_rd, n, d_jobs, d_syntax, d_opts,
                                 d_sjobs, d_ctx_in, d_cu_ctx_in, d_sresults, d_results, d_coef_out, d_reco_out, c->rqt_buf, c->rqt_bytes, nullptr, hop_intra_final_always());
}

int hop_intra_luma_search(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_intra_cu_syntax* syntax, const hop_intra_rqt_opt* opts, const hop_intra_search_job* sjobs,
                          int n_ctx, const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in, hop_intra_search_result* sresults, hop_rqt_result* results,
                          int32_t* coef_out, int16_t* reco_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !opts || !sjobs || !ctx_in || !cu_ctx_in || !sresults || !results || !coef_out || !reco_out || n_ctx <= 0)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_luma_search: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_luma_search: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0), roff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_intra_cu_syntax& y = syntax[i]; const hop_intra_search_job& s = sjobs[i];
    const int nxn = y.part_nxn ? 1 : 0;
    bool ok = rqt_class_ok(j) && cu_rect_ok(c, j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0 && j.qp_scaled[0] >= 0 && j.qp_scaled[0] <= 87 && j.lambda_rdoq[0] > 0.0 &&
              y.skip_ctx >= 0 && y.skip_ctx <= 2 && j.log2_cu - nxn >= j.log2_min_tu_in_cu && s.num_full_rd >= 1 && s.num_full_rd <= 8 && s.sqrt_lambda > 0.0;
    for (int p = 0; p < 4 && ok; p++) ok = s.left_dir[p] >= 0 && s.left_dir[p] < 35 && s.above_dir[p] >= 0 && s.above_dir[p] < 35;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra search job %d: illegal CU / transform-tree limits / neighbour directions / snapshot / parameters", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu); roff[i + 1] = roff[i] + ((size_t)1 << (2 * j.log2_cu));
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  auto same = [&](int p, int q) {
    return same_tree(jobs[p], jobs[q]) && !jobs[p].sign_hide == !jobs[q].sign_hide && !syntax[p].part_nxn == !syntax[q].part_nxn && sjobs[p].num_full_rd == sjobs[q].num_full_rd;
  };
  return for_each_class(n, same, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]]; const int nxn = syntax[idx[0]].part_nxn ? 1 : 0, nf = sjobs[idx[0]].num_full_rd;
    const size_t m = idx.size(), cu2 = (size_t)1 << (2 * f.log2_cu), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_intra_cu_syntax> sy = gather(syntax, idx); const std::vector<hop_intra_rqt_opt> op = gather(opts, idx);
    const std::vector<hop_intra_search_job> sj = gather(sjobs, idx);
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dp = a.in(op.data(), m); auto ds = a.in(sj.data(), m); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
    auto dq = a.out<hop_intra_search_result>(m); auto dr = a.out<hop_rqt_result>(m); auto d_co = a.out<int32_t>(m * cu3); auto dk = a.out<int16_t>(m * cu2);
    a.zero_span(dq, a.end_mark());                                     // every output starts cleared
    int r = a.commit(256); if (r) return r;
    r = hop_intra_luma_search_device(c, (int)m, a[dj], &f, nxn, nf, a[dy], a[dp], a[ds], a[dc], a[du], a[dq], a[dr], a[d_co], a[dk]); if (r) return r;
    std::vector<hop_intra_search_result> sr(m); std::vector<hop_rqt_result> rr(m); std::vector<int32_t> co(m * cu3); std::vector<int16_t> rk(m * cu2);
    if ((r = a.download(sr.data(), dq)) || (r = a.download(rr.data(), dr)) || (r = a.download(co.data(), d_co)) || (r = a.download(rk.data(), dk)) || (r = a.sync())) return r;
    scatter(sresults, idx, sr.data()); scatter(results, idx, rr.data());
    scatter(coef_out, idx, co.data(), cu3, coff.data()); scatter(reco_out, idx, rk.data(), cu2, roff.data());
    return (int)HOP_OK;
  });
}

int hop_intra_chroma_search_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, const hop_intra_cu_syntax* d_syntax, const hop_intra_rqt_opt* d_opts,
                                   const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in, hop_rqt_result* d_results, hop_intra_chroma_result* d_cresults,
                                   int32_t* d_coef_out, int16_t* d_reco_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_syntax || !d_opts || !d_ctx_in || !d_cu_ctx_in || !d_results || !d_cresults || !d_coef_out || !d_reco_out)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_chroma_search_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_chroma_search: hop_upload_orig has not been called");
  if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_chroma_search_device: illegal CU class");
  if (n == 0) return HOP_OK;
  int r = rqt_reserve(c, hop_intra_chroma_work_bytes(cls->log2_cu, n)); if (r) return r;
  return hop_launch_intra_chroma_search(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, n, d_jobs, d_syntax, d_opts, d_ctx_in,
                                        d_cu_ctx_in, d_results, d_cresults, d_coef_out, d_reco_out, c->rqt_buf, c->rqt_bytes, nullptr);
}

int hop_intra_chroma_search(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_intra_cu_syntax* syntax, const hop_intra_rqt_opt* opts, int n_ctx, const hop_cabac_ctx* ctx_in,
                            const hop_cabac_cu_ctx* cu_ctx_in, hop_rqt_result* results, hop_intra_chroma_result* cresults, int32_t* coef_out, int16_t* reco_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !opts || !ctx_in || !cu_ctx_in || !results || !cresults || !coef_out || !reco_out || n_ctx <= 0)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_chroma_search: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_chroma_search: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0), roff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_intra_cu_syntax& y = syntax[i];
    const int parts = 1 << (2 * (j.log2_cu - 2));
    bool ok = rqt_class_ok(j) && cu_rect_ok(c, j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0 && y.luma_dir[0] >= 0 && y.luma_dir[0] < 35;
    for (int k = 1; k < 3 && ok; k++) ok = j.qp_scaled[k] >= 0 && j.qp_scaled[k] <= 87 && j.lambda_rdoq[k] > 0.0;
    // the luma tree must be a legal tree of the class: every depth within the limits, quadrants consistent
    for (int p = 0; p < parts && ok; p++) {
      const int d = results[i].tr_idx[p], lg = j.log2_cu - d;
      ok = d >= 0 && d <= 3 && lg >= j.log2_min_tu_in_cu && lg <= j.log2_max_tu && results[i].tr_idx[p - p % (parts >> (2 * d))] == d && results[i].tskip[0][p] <= 1;
    }
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra chroma search job %d: illegal CU / transform-tree limits / luma tree / snapshot / parameters", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu); roff[i + 1] = roff[i] + ((size_t)1 << (2 * j.log2_cu - 1));
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  return for_each_class(n, [&](int p, int q) { return same_tree(jobs[p], jobs[q]) && !jobs[p].sign_hide == !jobs[q].sign_hide; }, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu2 = (size_t)1 << (2 * f.log2_cu), cu3 = cu_coeffs(f.log2_cu), h2x2 = cu2 >> 1;
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_intra_cu_syntax> sy = gather(syntax, idx); const std::vector<hop_intra_rqt_opt> op = gather(opts, idx);
    std::vector<hop_rqt_result> rr = gather(results, idx);
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dp = a.in(op.data(), m); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx); auto dr = a.in(rr.data(), m);
    auto dq = a.out<hop_intra_chroma_result>(m); auto d_co = a.out<int32_t>(m * cu3); auto dk = a.out<int16_t>(m * h2x2);
    a.zero_span(dq, a.end_mark());                                     // every output starts cleared
    int r = a.commit(256); if (r) return r;
    r = hop_intra_chroma_search_device(c, (int)m, a[dj], &f, a[dy], a[dp], a[dc], a[du], a[dr], a[dq], a[d_co], a[dk]); if (r) return r;
    std::vector<hop_intra_chroma_result> cr(m); std::vector<int32_t> co(m * cu3); std::vector<int16_t> rk(m * h2x2);
    if ((r = a.download(rr.data(), dr)) || (r = a.download(cr.data(), dq)) || (r = a.download(co.data(), d_co)) || (r = a.download(rk.data(), dk)) || (r = a.sync())) return r;
    scatter(results, idx, rr.data()); scatter(cresults, idx, cr.data());
    scatter(coef_out + cu2, idx, co.data() + cu2, cu2 >> 1, coff.data(), cu3);       // the chroma levels of the CU only
    scatter(reco_out, idx, rk.data(), h2x2, roff.data());
    return (int)HOP_OK;
  });
}

int hop_intra_cu_total_bits_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, const hop_intra_cu_syntax* d_syntax, const hop_rqt_result* d_results,
                                   const int32_t* d_coef, const uint32_t* d_dist, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in, uint32_t* d_bits, double* d_cost,
                                   hop_cabac_ctx* d_ctx_out, hop_cabac_cu_ctx* d_cu_ctx_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_syntax || !d_results || !d_coef || !d_ctx_in || !d_cu_ctx_in || !d_bits))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_total_bits_device: bad argument");
  if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_total_bits_device: illegal CU class");
  if (n == 0) return HOP_OK;
  return hop_launch_intra_cu_total(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, n, d_jobs, d_syntax, d_results, d_coef, d_ctx_in,
                                   d_cu_ctx_in, d_dist, d_bits, d_cost, d_ctx_out, d_cu_ctx_out);
}

int hop_intra_cu_total_bits(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_intra_cu_syntax* syntax, const hop_rqt_result* results, const int32_t* coef, const uint32_t* dist,
                            int n_ctx, const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in, uint32_t* bits, double* cost, hop_cabac_ctx* ctx_out,
                            hop_cabac_cu_ctx* cu_ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !results || !coef || !dist || !ctx_in || !cu_ctx_in || !bits || !cost || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_total_bits: bad argument");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_intra_cu_syntax& y = syntax[i];
    const int parts = 1 << (2 * (j.log2_cu - 2));
    bool ok = rqt_class_ok(j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0 && y.skip_ctx >= 0 && y.skip_ctx <= 2;
    for (int p = 0; p < (y.part_nxn ? 4 : 1) && ok; p++) ok = y.luma_dir[p] >= 0 && y.luma_dir[p] < 35 && y.pred_num[p] >= 0 && y.pred_num[p] <= 3;
    for (int p = 0; p < parts && ok; p++) {
      const int d = results[i].tr_idx[p], lg = j.log2_cu - d;
      ok = d >= (y.part_nxn ? 1 : 0) && d <= 3 && lg >= j.log2_min_tu_in_cu && lg <= j.log2_max_tu && results[i].tr_idx[p - p % (parts >> (2 * d))] == d;
    }
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "intra CU bits job %d: illegal CU class / syntax elements / transform tree / snapshot", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  return for_each_class(n, [&](int p, int q) { return same_tree(jobs[p], jobs[q]) && !jobs[p].sign_hide == !jobs[q].sign_hide; }, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_intra_cu_syntax> sy = gather(syntax, idx); const std::vector<hop_rqt_result> rr = gather(results, idx);
    const std::vector<int32_t> co = gather(coef, idx, cu3, coff.data()); const std::vector<uint32_t> dd = gather(dist, idx);
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dr = a.in(rr.data(), m); auto d_co = a.in(co.data(), m * cu3); auto d_di = a.in(dd.data(), m);
    auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
    auto db = a.out<uint32_t>(m); auto dk = a.out<double>(m); auto dx = a.out<hop_cabac_ctx>(m); auto dv = a.out<hop_cabac_cu_ctx>(m);
    a.end_mark();
    int r = a.commit(256); if (r) return r;
    r = hop_intra_cu_total_bits_device(c, (int)m, a[dj], &f, a[dy], a[dr], a[d_co], a[d_di], a[dc], a[du], a[db], a[dk], a[dx], a[dv]); if (r) return r;
    std::vector<uint32_t> bb(m); std::vector<double> kk(m); std::vector<hop_cabac_ctx> cx(m); std::vector<hop_cabac_cu_ctx> cv(m);
    if ((r = a.download(bb.data(), db)) || (r = a.download(kk.data(), dk)) || (r = a.download(cx.data(), dx)) || (r = a.download(cv.data(), dv)) || (r = a.sync())) return r;
    scatter(bits, idx, bb.data()); scatter(cost, idx, kk.data());
    if (ctx_out) scatter(ctx_out, idx, cx.data());
    if (cu_ctx_out) scatter(cu_ctx_out, idx, cv.data());
    return (int)HOP_OK;
  });
}

int hop_inter_cu_skip_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_cu_syntax* d_syntax, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in,
                             hop_cu_final* d_finals, uint32_t* d_bits, double* d_cost, hop_cabac_ctx* d_ctx_out, hop_cabac_cu_ctx* d_cu_ctx_out) {
  if (!c || n < 0 || (n && (!d_jobs || !d_syntax || !d_ctx_in || !d_cu_ctx_in || !d_finals || !d_bits || !d_cost))) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_skip_device: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_inter_cu_skip: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  return hop_launch_cu_skip(c, n, d_jobs, d_syntax, d_ctx_in, d_cu_ctx_in, d_finals, d_bits, d_cost, d_ctx_out, d_cu_ctx_out);
}

int hop_inter_cu_skip(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_cu_syntax* syntax, int n_ctx, const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in,
                      hop_cu_final* finals, uint32_t* bits, double* cost, hop_cabac_ctx* ctx_out, hop_cabac_cu_ctx* cu_ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !ctx_in || !cu_ctx_in || !finals || !bits || !cost || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_skip: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_inter_cu_skip: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_cu_syntax& y = syntax[i];
    const bool ok = cu_rect_ok(c, j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && j.lambda_rd > 0.0 && y.skip_ctx >= 0 && y.skip_ctx <= 2 && y.max_merge_cand >= 1 && y.max_merge_cand <= 5 &&
                    y.pu[0].merge_idx >= 0 && y.pu[0].merge_idx < y.max_merge_cand;
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "skip candidate %d: illegal CU / snapshot / merge index / parameters", i);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dy = a.in(syntax, n); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
  auto df = a.out<hop_cu_final>(n); auto db = a.out<uint32_t>(n); auto dk = a.out<double>(n); auto dx = a.out<hop_cabac_ctx>(n); auto dv = a.out<hop_cabac_cu_ctx>(n);
  a.end_mark();
  int r = a.commit(256); if (r) return r;
  r = hop_inter_cu_skip_device(c, n, a[dj], a[dy], a[dc], a[du], a[df], a[db], a[dk], a[dx], a[dv]); if (r) return r;
  if ((r = a.download(finals, df)) || (r = a.download(bits, db)) || (r = a.download(cost, dk))) return r;
  if (ctx_out && (r = a.download(ctx_out, dx))) return r;
  if (cu_ctx_out && (r = a.download(cu_ctx_out, dv))) return r;
  return a.sync();
}

// one class of intra candidates, device-resident from the rough search to the cost: luma search -> chroma search -> bits and cost, no host step in between
static int intra_candidate_chain(hop_ctx* c, const hop_intra_class& k, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in) {
  const hop_rqt_job* cls = &k.cls;
  const int nxn = k.part_nxn ? 1 : 0;
  if (k.n < 0 || (k.n && (!k.d_jobs || !k.d_syntax || !k.d_opts || !k.d_sjobs || !k.d_sresults || !k.d_results || !k.d_cresults || !k.d_coef || !k.d_reco_y || !k.d_reco_c ||
                          !k.d_syntax_out || !k.d_dist || !k.d_bits || !k.d_cost)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_device_classes: bad class descriptor");
  if (!rqt_class_ok(*cls) || cls->log2_cu - nxn < cls->log2_min_tu_in_cu || k.num_full_rd < 1 || k.num_full_rd > 8)
    return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_device_classes: illegal CU class");
  if (k.n == 0) return HOP_OK;
  if (k.n <= c->walk_max && !getenv("HOP_WALK_NO_INTRA")) {              // the RD spine's batches: one kernel per candidate (k_walk.inl)
    int r = walk_reserve(c, hop_intra_walk_bytes(c, cls->log2_cu, k.n, k.num_full_rd)); if (r) return r;
    return hop_launch_intra_walk(c, k, d_ctx_in, d_cu_ctx_in, c->walk_buf, c->walk_bytes);
  }
  int r = rqt_reserve(c, std::max(hop_intra_search_work_bytes(cls->log2_cu, k.n), hop_intra_chroma_work_bytes(cls->log2_cu, k.n))); if (r) return r;
  const int sh = cls->sign_hide ? 1 : 0, ts = cls->use_ts ? 1 : 0;
  r = hop_launch_intra_search(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, sh, ts, nxn, k.num_full_rd, k.n, k.d_jobs, k.d_syntax, k.d_opts, k.d_sjobs, d_ctx_in, d_cu_ctx_in,
                              k.d_sresults, k.d_results, k.d_coef, k.d_reco_y, c->rqt_buf, c->rqt_bytes, k.d_syntax_out, hop_intra_final_always());
  if (r) return r;
  r = hop_launch_intra_chroma_search(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, sh, ts, k.n, k.d_jobs, k.d_syntax_out, k.d_opts, d_ctx_in, d_cu_ctx_in, k.d_results,
                                     k.d_cresults, k.d_coef, k.d_reco_c, c->rqt_buf, c->rqt_bytes, k.d_syntax_out);
  if (r) return r;
  r = hop_launch_intra_dist_sum(c, k.n, k.d_sresults, k.d_cresults, k.d_dist);
  if (r) return r;
  // the chroma direction of the winner goes into the syntax elements before the bits are counted
  return hop_launch_intra_cu_total(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, sh, ts, k.n, k.d_jobs, k.d_syntax_out, k.d_results, k.d_coef, d_ctx_in, d_cu_ctx_in, k.d_dist,
                                   k.d_bits, k.d_cost, k.d_ctx_out, k.d_cu_ctx_out);
}

int hop_intra_cu_device_classes(hop_ctx* c, int n_classes, const hop_intra_class* classes, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in) {
  if (!c || n_classes < 0 || (n_classes && (!classes || !d_ctx_in || !d_cu_ctx_in))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_cu_device_classes: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_intra_cu_device_classes: hop_upload_orig has not been called");
  if (n_classes == 0) return HOP_OK;
  return run_on_lanes(c, n_classes, "hop_intra_cu_device_classes", [&](int i) { return intra_candidate_chain(c, classes[i], d_ctx_in, d_cu_ctx_in); });
}

static int inter_candidate_chain(hop_ctx* c, const hop_inter_class& k, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in) {
  if (k.n < 0 || (k.n && (!k.d_jobs || !k.d_syntax || !k.d_results || !k.d_coef || !k.d_ctx_after || !k.d_finals || !k.d_bits || !k.d_skipped || !k.d_cost)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_device_classes: bad class descriptor");
  if (k.n == 0) return HOP_OK;
  if (k.n <= c->walk_max && !getenv("HOP_WALK_NO_INTER")) {              // the RD spine's batches: one kernel per candidate (k_walk.inl)
    const hop_rqt_job* cls = &k.cls;
    if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_device_classes: illegal CU class");
    if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_inter_cu_device_classes: hop_upload_orig has not been called");
    int r = walk_reserve(c, hop_inter_walk_bytes(cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, k.n)); if (r) return r;
    return hop_launch_inter_walk(c, cls, k.n, k.d_jobs, k.d_syntax, d_ctx_in, d_cu_ctx_in, k.d_results, k.d_coef, k.d_ctx_after, k.d_finals, k.d_bits, k.d_skipped, k.d_cost, k.d_ctx_out,
                                 k.d_cu_ctx_out, c->walk_buf, c->walk_bytes);
  }
  int r = hop_rqt_device(c, k.n, k.d_jobs, &k.cls, d_ctx_in, k.d_results, k.d_coef, k.d_ctx_after); if (r) return r;
  r = hop_rqt_finish_device(c, k.n, k.d_jobs, &k.cls, k.d_results, k.d_coef, k.d_ctx_after, k.d_finals); if (r) return r;
  r = hop_inter_cu_bits_device(c, k.n, k.d_jobs, &k.cls, k.d_syntax, k.d_results, k.d_coef, d_ctx_in, d_cu_ctx_in, k.d_bits, k.d_skipped, k.d_ctx_out, k.d_cu_ctx_out); if (r) return r;
  return hop_launch_inter_cost(c, k.n, k.d_jobs, k.d_finals, k.d_bits, k.d_cost);
}

int hop_inter_cu_device_classes(hop_ctx* c, int n_classes, const hop_inter_class* classes, const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in) {
  if (!c || n_classes < 0 || (n_classes && (!classes || !d_ctx_in || !d_cu_ctx_in))) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_device_classes: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_inter_cu_device_classes: hop_upload_orig has not been called");
  if (n_classes == 0) return HOP_OK;
  return run_on_lanes(c, n_classes, "hop_inter_cu_device_classes", [&](int i) { return inter_candidate_chain(c, classes[i], d_ctx_in, d_cu_ctx_in); });
}

int hop_inter_cu_bits_device(hop_ctx* c, int n, const hop_rqt_job* d_jobs, const hop_rqt_job* cls, const hop_cu_syntax* d_syntax, const hop_rqt_result* d_results, const int32_t* d_coef,
                             const hop_cabac_ctx* d_ctx_in, const hop_cabac_cu_ctx* d_cu_ctx_in, uint32_t* d_bits, uint32_t* d_skipped, hop_cabac_ctx* d_ctx_out,
                             hop_cabac_cu_ctx* d_cu_ctx_out) {
  if (!c || n < 0 || !cls || (n && (!d_jobs || !d_syntax || !d_results || !d_coef || !d_ctx_in || !d_cu_ctx_in || !d_bits || !d_skipped)))
    return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_bits_device: bad argument");
  if (!rqt_class_ok(*cls)) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_bits_device: illegal CU class");
  if (n == 0) return HOP_OK;
  return hop_launch_cu_bits(c, cls->log2_cu, cls->log2_max_tu, cls->log2_min_tu_in_cu, cls->inter_split_flag ? 1 : 0, cls->sign_hide ? 1 : 0, cls->use_ts ? 1 : 0, n, d_jobs, d_syntax,
                            d_results, d_coef, d_ctx_in, d_cu_ctx_in, d_bits, d_skipped, d_ctx_out, d_cu_ctx_out);
}

int hop_inter_cu_bits(hop_ctx* c, int n, const hop_rqt_job* jobs, const hop_cu_syntax* syntax, const hop_rqt_result* results, const int32_t* coef, int n_ctx,
                      const hop_cabac_ctx* ctx_in, const hop_cabac_cu_ctx* cu_ctx_in, uint32_t* bits, uint32_t* skipped, hop_cabac_ctx* ctx_out, hop_cabac_cu_ctx* cu_ctx_out) {
  if (!c || n < 0 || (n && (!jobs || !syntax || !results || !coef || !ctx_in || !cu_ctx_in || !bits || !skipped || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_inter_cu_bits: bad argument");
  if (n == 0) return HOP_OK;
  std::vector<size_t> coff(n + 1, 0);
  for (int i = 0; i < n; i++) {
    const hop_rqt_job& j = jobs[i]; const hop_cu_syntax& y = syntax[i];
    bool ok = rqt_class_ok(j) && j.ctx_index >= 0 && j.ctx_index < n_ctx && y.part_size >= 0 && y.part_size <= 7 &&
              y.n_pu == (y.part_size == 0 ? 1 : y.part_size == 3 ? 4 : 2) && y.skip_ctx >= 0 && y.skip_ctx <= 2 && y.max_merge_cand >= 1 && y.max_merge_cand <= 5;
    for (int p = 0; p < y.n_pu && ok; p++) ok = y.pu[p].merge_flag ? (y.pu[p].merge_idx >= 0 && y.pu[p].merge_idx < 5) : (y.pu[p].mvp_idx >= 0 && y.pu[p].mvp_idx <= 1);
    if (!ok) return hop_set_err(c, HOP_ERR_ARG, "CU bits job %d: illegal CU class / syntax elements / snapshot", i);
    coff[i + 1] = coff[i] + cu_coeffs(j.log2_cu);
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, cu_ctx_in)) return HOP_ERR_ARG;
  auto same = [&](int p, int q) { return same_tree(jobs[p], jobs[q]) && !jobs[p].inter_split_flag == !jobs[q].inter_split_flag && !jobs[p].sign_hide == !jobs[q].sign_hide; };
  return for_each_class(n, same, [&](const std::vector<int>& idx) {
    const hop_rqt_job& f = jobs[idx[0]];
    const size_t m = idx.size(), cu3 = cu_coeffs(f.log2_cu);
    const std::vector<hop_rqt_job> cls = gather(jobs, idx); const std::vector<hop_cu_syntax> sy = gather(syntax, idx); const std::vector<hop_rqt_result> rr = gather(results, idx);
    const std::vector<int32_t> co = gather(coef, idx, cu3, coff.data());
    stage_arena a(c);
    auto dj = a.in(cls.data(), m); auto dy = a.in(sy.data(), m); auto dr = a.in(rr.data(), m); auto d_co = a.in(co.data(), m * cu3); auto dc = a.in(ctx_in, n_ctx); auto du = a.in(cu_ctx_in, n_ctx);
    auto db = a.out<uint32_t>(m); auto ds = a.out<uint32_t>(m); auto dx = a.out<hop_cabac_ctx>(m); auto dv = a.out<hop_cabac_cu_ctx>(m);
    a.end_mark();
    int r = a.commit(256); if (r) return r;
    r = hop_launch_cu_bits(c, f.log2_cu, f.log2_max_tu, f.log2_min_tu_in_cu, f.inter_split_flag ? 1 : 0, f.sign_hide ? 1 : 0, f.use_ts ? 1 : 0, (int)m, a[dj], a[dy], a[dr], a[d_co], a[dc], a[du],
                           a[db], a[ds], a[dx], a[dv]);
    if (r) return r;
    std::vector<uint32_t> bb(m), ss(m); std::vector<hop_cabac_ctx> cx(m); std::vector<hop_cabac_cu_ctx> cv(m);
    if ((r = a.download(bb.data(), db)) || (r = a.download(ss.data(), ds)) || (r = a.download(cx.data(), dx)) || (r = a.download(cv.data(), dv)) || (r = a.sync())) return r;
    scatter(bits, idx, bb.data()); scatter(skipped, idx, ss.data());
    if (ctx_out) scatter(ctx_out, idx, cx.data());
    if (cu_ctx_out) scatter(cu_ctx_out, idx, cv.data());
    return (int)HOP_OK;
  });
}

int hop_tu_rd(hop_ctx* c, int n, const hop_tu_rd_job* jobs, int n_ctx, const hop_cabac_ctx* ctx_in, hop_tu_rd_result* results, int32_t* levels_out) {
  if (!c || n < 0 || (n && (!jobs || !ctx_in || !results || !levels_out || n_ctx <= 0))) return hop_set_err(c, HOP_ERR_ARG, "hop_tu_rd: bad argument");
  if (!c->have_orig) return hop_set_err(c, HOP_ERR_STATE, "hop_tu_rd: hop_upload_orig has not been called");
  if (n == 0) return HOP_OK;
  std::vector<int64_t> offs(n);
  size_t tot = 0;
  for (int i = 0; i < n; i++) {
    const hop_tu_rd_job& j = jobs[i];
    const int N = 1 << j.log2_size, sh = j.comp ? 1 : 0;
    if (j.comp < 0 || j.comp > 2 || j.log2_size < 2 || j.log2_size > 5 || (j.comp && j.log2_size == 5) || j.x < 0 || j.y < 0 || ((j.x >> sh) & 3) || ((j.y >> sh) & 3) ||
        (j.x >> sh) + N > (c->pic_w >> sh) || (j.y >> sh) + N > (c->pic_h >> sh) || j.qp_scaled < 0 || j.qp_scaled > 87 || j.tr_depth < 0 || j.tr_depth > 3 ||
        j.ctx_index < 0 || j.ctx_index >= n_ctx || j.bit_depth != (j.comp ? c->bd_c : c->bd_y) || !(j.lambda_rdoq > 0.0) || !(j.lambda_rd > 0.0) ||
        j.scan_idx < 0 || j.scan_idx > 2 || (!j.is_intra && (j.scan_idx || j.use_dst)) || (j.flags & ~3) ||
        ((j.flags & HOP_TU_RD_TS) && (j.log2_size != 2 || !j.use_ts)))
      return hop_set_err(c, HOP_ERR_ARG, "TU RD job %d: illegal transform unit / snapshot / parameters", i);
    offs[i] = (int64_t)tot; tot += (size_t)N * N;
  }
  if (!ctx_states_ok(c, n_ctx, ctx_in, nullptr)) return HOP_ERR_ARG;
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dc = a.in(ctx_in, n_ctx); auto d_off = a.in(offs.data(), n); auto dl = a.out<int32_t>(tot); auto dr = a.out<hop_tu_rd_result>(n);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_tu_rd(c, n, a[dj], a[dc], a[d_off], tot, a[dl], a[dr], 0); if (r) return r;
  if ((r = a.download(results, dr)) || (r = a.download(levels_out, dl))) return r;
  return a.sync();
}

int hop_intra_pred(hop_ctx* c, int n, const hop_intra_job* jobs, const int32_t* modes) {
  if (!c || n < 0 || (n && (!jobs || !modes))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_pred: bad argument");
  if (n == 0) return HOP_OK;
  int u = 0;
  for (int i = 0; i < n; i++) {
    if (!intra_block_ok(c, jobs[i], 0) || modes[i] < 0 || modes[i] > 34) return hop_set_err(c, HOP_ERR_ARG, "intra pred job %d: illegal block or mode", i);
    if (!intra_neighbours_ok(c, jobs[i], 0, &u)) return hop_set_err(c, HOP_ERR_ARG, "intra pred job %d: neighbour unit %d flagged available but outside the picture", i, u);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dm = a.in(modes, n);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_intra_pred(c, n, a[dj], a[dm]); if (r) return r;
  return a.sync();
}
int hop_intra_pred_chroma(hop_ctx* c, int n, const hop_intra_job* jobs, const int32_t* modes) {
  if (!c || n < 0 || (n && (!jobs || !modes))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_pred_chroma: bad argument");
  if (n == 0) return HOP_OK;
  int u = 0;
  for (int i = 0; i < n; i++) {
    if (!intra_block_ok(c, jobs[i], 1) || modes[i] < 0 || modes[i] > 34) return hop_set_err(c, HOP_ERR_ARG, "chroma intra pred job %d: illegal block or mode", i);
    if (!intra_neighbours_ok(c, jobs[i], 1, &u)) return hop_set_err(c, HOP_ERR_ARG, "chroma intra pred job %d: neighbour unit %d flagged available but outside the picture", i, u);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto dm = a.in(modes, n);
  int r = a.commit(256); if (r) return r;
  r = hop_launch_intra_pred_chroma(c, n, a[dj], a[dm]); if (r) return r;
  return a.sync();
}
int hop_intra_pred_chroma_device(hop_ctx* c, int n, const hop_intra_job* d_jobs, const int32_t* d_modes) {
  if (!c || n < 0 || (n && (!d_jobs || !d_modes))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_pred_chroma_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_intra_pred_chroma(c, n, d_jobs, d_modes);
}
int hop_intra_pred_device(hop_ctx* c, int n, const hop_intra_job* d_jobs, const int32_t* d_modes) {
  if (!c || n < 0 || (n && (!d_jobs || !d_modes))) return hop_set_err(c, HOP_ERR_ARG, "hop_intra_pred_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_intra_pred(c, n, d_jobs, d_modes);
}

int hop_distortion_device(hop_ctx* c, int n, const hop_dist_job* d_jobs, uint32_t* d_out) {
  if (!c || n < 0 || (n && (!d_jobs || !d_out))) return hop_set_err(c, HOP_ERR_ARG, "hop_distortion_device: bad argument");
  if (n == 0) return HOP_OK;
  return hop_launch_dist(c, n, d_jobs, d_out);
}

int hop_distortion(hop_ctx* c, int n, const hop_dist_job* jobs, uint32_t* out) {
  if (!c || n < 0 || (n && (!jobs || !out))) return hop_set_err(c, HOP_ERR_ARG, "hop_distortion: bad argument");
  if (n == 0) return HOP_OK;
  for (int i = 0; i < n; i++) {
    const hop_dist_job& j = jobs[i];
    if (j.comp < 0 || j.comp > 2 || j.kind < 0 || j.kind > 2 || j.x < 0 || j.y < 0 || j.w <= 0 || j.h <= 0 || (j.w & 3) || (j.h & 3) || j.x + j.w > c->pic_w || j.y + j.h > c->pic_h)
      return hop_set_err(c, HOP_ERR_ARG, "dist job %d: bad rectangle/kind", i);
  }
  stage_arena a(c);
  auto dj = a.in(jobs, n); auto d_o = a.out<uint32_t>(n);
  int r = a.commit(0); if (r) return r;
  r = hop_launch_dist(c, n, a[dj], a[d_o]); if (r) return r;
  r = a.download(out, d_o); if (r) return r;
  return a.sync();
}

} // extern "C"
