// k_stream.hip -- hop_access_unit_write, hop_rbsp_escape, hop_picture_hash: the outer layer of the stream on the device.  The syntax (parameter sets, slice header,
// SEI, NAL framing) is host/hop_stream.cpp; here are the two passes over data that already lives in HBM: emulation prevention over the packed substreams (replaces the
// loop of write(), TLibEncoder/NALwrite.cpp:108-152, and TComOutputBitstream::countStartCodeEmulations, TLibCommon/TComBitStream.cpp:186-216) and the picture checksum
// (compChecksum, TLibCommon/TComPicYuvMD5.cpp:141-164).
//
// Emulation prevention as a scan.  With z(i) = the number of zero bytes immediately in front of byte i, the sequential rule (a counter of zeros, 03 in front of a byte
// <= 3 when the counter is 2, the counter reset by the insertion) puts an 03 in front of byte i exactly when z(i) >= 2, z(i) is even and byte i <= 3: inside a run
// of zeros that starts at s the insertions fall in front of s + 2, s + 4, ..., and in front of the byte that ends the run when its length is even and that byte is <= 3.
// z(i) needs only the position of the last non-zero byte in front of i, which is a max-scan.  A chunk of 4096 bytes (256 lanes x 16) knows it for every byte behind its
// own first non-zero byte; for the zeros it starts with, z(i) = i - chunk start + carry, and of the carry (the zeros in front of the chunk) only 0 / 1 / ">= 2 and even" /
// ">= 2 and odd" matters.  So:
//   k_esc_count    per chunk: the insertions behind its first non-zero byte, the insertions among its leading bytes for each of the four carries, the position of its
//                  last non-zero byte.  ISOLATED: every segment start counts as a non-zero byte in front of it (the count of a segment ALONE, which is what the entry
//                  points take), and the carry-free part goes to the segment's word by atomicAdd
//   k_esc_scan     one block per job over the chunk records: each chunk's carry (max-scan of the last non-zero positions) and output offset (sum-scan of the counts the
//                  carry selects), the total with the final 03 behind a trailing 00.  ISOLATED: the leading part the carry selects is added to its segment's word
//   k_esc_scatter  the flags again with the carry known, an exclusive prefix over the lanes (wave scan, then across the four waves through LDS), the bytes and the 03s
//                  stored below the capacity only
// The input of a job is a virtual concatenation -- `head` (the uploaded NAL and slice header), then `body` (the substreams where k_entropy_pack left them): no copy.
// Jobs (pictures of a stack) are the grid's y dimension.  An all-zero buffer costs what random bytes cost: no lane looks back further than its chunk.
// No kernel looks at another workgroup's progress.
// The way back -- hop_rbsp_unescape, hop_access_unit_read, hop_access_unit_decode -- is further down: k_une_count / k_une_scan / k_une_compact remove emulation
// prevention (the syntax is host/hop_stream_read.cpp), and the decode entry hands the compact kernel's output to the parser's kernels (csrc/k_parse.hip).
// hop_access_units_decode, at the end, does it for the n pictures of a stacked context at once, the access units as the unescape grid's y dimension.
#include <string.h>
#include <algorithm>
#include <vector>
#include "hop_dev.h"

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hop_set_err((c), HOP_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

extern "C" {
int hop_ent_write_device(hop_ctx* c, const hop_slice_data_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao, uint8_t* out,
                         size_t out_capacity, uint32_t* substream_bytes, int32_t* n_substreams, size_t reserve, const uint8_t** d_packed, uint8_t** d_reserve,
                         const int32_t* pic_qp);                                                                                                              // k_entropy.hip
int hop_strm_check(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, char* err, size_t errn);                                                  // host/hop_stream.cpp
void hop_strm_parameter_sets(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, std::vector<uint8_t>& s);
void hop_strm_slice_header(int pic_w, int pic_h, const hop_stream_params* p, const uint32_t* sub_bytes, const uint32_t* sub_emul, int n_sub, std::vector<uint8_t>& s);
void hop_strm_sei(int method, const uint8_t digest[3][16], std::vector<uint8_t>& s);
void hop_strm_hash_plane(int method, int bit_depth, const int16_t* plane, int w, int h, size_t stride, uint8_t digest[16]);
size_t hop_parse_work_bytes(const hop_ctx* c, size_t data_bytes, int n_substreams);                                                                         // k_parse.hip
int hop_parse_device(hop_ctx* c, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data, const uint32_t* substream_bytes, int32_t n_substreams,
                     hop_cu_part* parts, int32_t* levels, hop_sao_param* sao, size_t front, const int32_t* pic_qp);
struct hop_parse_where { const hop_cu_part* d_parts; const int32_t* d_levels; size_t end; };
int hop_parse_device_at(hop_ctx* c, const char* who, const char* noun, const hop_slice_data_params* p, const uint8_t* data, const uint8_t* d_data, const unsigned long long* offsets,
                        const uint32_t* substream_bytes, int32_t n_substreams, hop_cu_part* parts, int32_t* levels, hop_sao_param* sao, size_t front, hop_parse_where* where,
                        const int32_t* pic_qp);
int hop_dec_device(hop_ctx* c, const char* who, const char* noun, const hop_dec_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_cu_part* d_parts, const int32_t* d_levels,
                   int32_t* d_order, const int32_t* pic_qp);                                                                                                  // k_decode.hip
int hop_dbk_device(hop_ctx* c, const hop_deblock_params* p, const hop_cu_part* parts, const int32_t* pic_qp);                                                 // k_deblock.hip
}
#include "../host/hop_stream_read.h"

namespace {
constexpr int ESC_LANE = 16, ESC_THREADS = 256, ESC_CHUNK = ESC_LANE * ESC_THREADS;

struct EscRec {                    // one chunk
  uint32_t lead[4];                // insertions among the bytes in front of the chunk's first non-zero byte (or segment start), for a carry of 0, 1, >= 2 even, >= 2 odd
  uint32_t local;                  // insertions behind it
  int32_t  last;                   // position in the chunk of its last non-zero byte (ISOLATED: or of the byte in front of its last segment start); -1: none
  uint32_t lead_seg;               // ISOLATED: the segment the chunk starts in
  uint32_t carry;                  // from the scan: 0, 1, 2 (>= 2, even), 3 (>= 2, odd)
  unsigned long long out_off;      // from the scan: where the chunk's first byte (or the 03 in front of it) goes
};
struct EscJob {
  const uint8_t* head; const uint8_t* body; uint32_t head_len, total;      // the input: head[0 .. head_len), then body[0 .. total - head_len)
  const uint32_t* seg_end; uint32_t n_seg; uint32_t* seg_cnt;              // ISOLATED: the segments' end positions (ascending, the last = total), their counts
  EscRec* recs; uint32_t n_chunks;
  uint8_t* out; unsigned long long out_cap; unsigned long long* out_total;
};

// the lane's 16 bytes from position `at` (zeros behind the end)
__device__ static inline void esc_load(const EscJob& J, uint32_t at, uint8_t v[ESC_LANE]) {
  if (at + ESC_LANE <= J.total && (at >= J.head_len || at + ESC_LANE <= J.head_len)) {
    const uint8_t* p = at >= J.head_len ? J.body + (at - J.head_len) : J.head + at;
    __builtin_memcpy(v, p, ESC_LANE);
  } else {
#pragma unroll
    for (int j = 0; j < ESC_LANE; j++) { const uint32_t i = at + j; v[j] = i < J.total ? (i < J.head_len ? J.head[i] : J.body[i - J.head_len]) : 0; }
  }
}
__device__ static inline uint32_t esc_segment_of(const EscJob& J, uint32_t pos) {   // the first segment whose end lies behind pos
  uint32_t lo = 0, hi = J.n_seg - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (J.seg_end[mid] > pos) hi = mid; else lo = mid + 1; }
  return lo;
}
__device__ static inline int esc_flag(int zeros, uint8_t b) { return zeros >= 2 && !(zeros & 1) && b <= 3; }
// exclusive max-scan over the block's 256 lanes (-1 in front of lane 0); part: 4 ints of LDS, which hold the four waves' maxima afterwards
__device__ static inline int esc_block_max_before(int v, int* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v = max(v, t); }
  if (lane == 63) part[wave] = v;
  int before = __shfl_up(v, 1, 64);
  if (lane == 0) before = -1;
  __syncthreads();
  for (int w = 0; w < wave; w++) before = max(before, part[w]);
  return before;
}
__device__ static inline uint32_t esc_block_sum_scan(uint32_t v, uint32_t* part) {   // inclusive
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  if (lane == 63) part[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; w++) v += part[w];
  __syncthreads();
  return v;
}

// what a lane knows in front of its first byte: `prev` = the position in the chunk of the last non-zero byte (or segment boundary) in front of it, -1 when that is the
// byte in front of the chunk for certain (the data's or, ISOLATED, a segment's start), PREV_CARRY when it lies in front of the chunk: then z = position + carry
constexpr int PREV_CARRY = -2;

template <bool ISOLATED>
__global__ __launch_bounds__(ESC_THREADS) void k_esc_count(const EscJob* __restrict__ jobs) {
  __shared__ int part[4];
  __shared__ uint32_t sums[4][6];
  const EscJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks) return;                                  // (uniform: the whole block)
  const uint32_t chunk = blockIdx.x * (uint32_t)ESC_CHUNK;
  const int t = threadIdx.x, rel0 = t * ESC_LANE;
  uint8_t v[ESC_LANE];
  esc_load(J, chunk + rel0, v);
  const int n_valid = (int)min((uint32_t)ESC_LANE, J.total - min(J.total, chunk + rel0));
  int own = -1;                                                          // the lane's last non-zero byte
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) if (j < n_valid && v[j]) own = rel0 + j;
  uint32_t seg = 0, seg_stop = J.total;                                  // ISOLATED: the segment of the lane's current byte and where it ends
  if (ISOLATED && n_valid) {
    seg = esc_segment_of(J, chunk + rel0); seg_stop = J.seg_end[seg];
    // a segment that starts behind the lane's first byte, up to the next lane's first: the byte in front of it counts as non-zero (for the lanes and chunks behind)
    for (uint32_t s = seg, e = seg_stop; e < J.total && e <= chunk + rel0 + ESC_LANE; e = J.seg_end[++s]) own = max(own, (int)(e - chunk) - 1);
  }
  int prev = esc_block_max_before(own, part);
  if (prev < 0) prev = chunk == 0 ? -1 : PREV_CARRY;                     // nothing in front inside the chunk
  if (ISOLATED && n_valid) {                                             // the start of the lane's own segment, when the chunk holds it
    const uint32_t start = seg ? J.seg_end[seg - 1] : 0u;
    if (start >= chunk) prev = max(prev, (int)(start - chunk) - 1);
  }
  uint32_t lead[4] = { 0, 0, 0, 0 }, local = 0, acc = 0;
  const bool one_segment = !ISOLATED || esc_segment_of(J, chunk) == esc_segment_of(J, min(J.total, chunk + (uint32_t)ESC_CHUNK) - 1);
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) {
    if (j >= n_valid) continue;
    const int rel = rel0 + j;
    if (ISOLATED && chunk + rel == seg_stop) {                           // a segment starts here
      if (!one_segment && acc) atomicAdd(&J.seg_cnt[seg], acc);
      acc = 0; seg++; seg_stop = J.seg_end[min(seg, J.n_seg - 1)]; prev = rel - 1;
    }
    if (prev == PREV_CARRY) {
#pragma unroll
      for (int c = 0; c < 4; c++) lead[c] += esc_flag(rel + c, v[j]);
    } else {
      const int f = esc_flag(rel - 1 - prev, v[j]);
      local += f; acc += f;
    }
    if (v[j]) prev = rel;
  }
  if (ISOLATED && !one_segment && acc && n_valid) atomicAdd(&J.seg_cnt[min(seg, J.n_seg - 1)], acc);
  // the block's sums: lead[0..3], local, and for one_segment the same local into the segment's word
  uint32_t s5[5] = { lead[0], lead[1], lead[2], lead[3], local };
#pragma unroll
  for (int k = 0; k < 5; k++) {
    uint32_t x = s5[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((t & 63) == 0) sums[t >> 6][k] = x;
  }
  __syncthreads();
  if (t == 0) {
    EscRec r;
    for (int k = 0; k < 4; k++) r.lead[k] = sums[0][k] + sums[1][k] + sums[2][k] + sums[3][k];
    r.local = sums[0][4] + sums[1][4] + sums[2][4] + sums[3][4];
    r.last = part[0] > part[1] ? part[0] : part[1]; r.last = max(r.last, max(part[2], part[3]));
    r.lead_seg = ISOLATED ? esc_segment_of(J, chunk) : 0; r.carry = 0; r.out_off = 0;
    J.recs[blockIdx.x] = r;
    if (ISOLATED && one_segment && r.local) atomicAdd(&J.seg_cnt[r.lead_seg], r.local);
  }
}

template <bool ISOLATED>
__global__ __launch_bounds__(ESC_THREADS) void k_esc_scan(const EscJob* __restrict__ jobs) {
  __shared__ long long mx[ESC_THREADS];
  __shared__ unsigned long long sm[ESC_THREADS];
  const EscJob J = jobs[blockIdx.x];
  const int t = threadIdx.x;
  long long run_last = -1;                                               // the last non-zero position in front of the tile (-1: the data's start)
  unsigned long long run_sum = 0;                                        // insertions in front of the tile
  for (uint32_t base = 0; base < J.n_chunks; base += ESC_THREADS) {
    const uint32_t k = base + t;
    const bool on = k < J.n_chunks;
    EscRec r; r.last = -1; r.local = 0; r.lead[0] = r.lead[1] = r.lead[2] = r.lead[3] = 0; r.lead_seg = 0;
    if (on) r = J.recs[k];
    const long long mine = on && r.last >= 0 ? (long long)k * ESC_CHUNK + r.last : -1;
    mx[t] = mine;
    __syncthreads();
    for (int o = 1; o < ESC_THREADS; o <<= 1) {                           // inclusive max-scan
      const long long a = t >= o ? mx[t - o] : -1;
      __syncthreads();
      if (a > mx[t]) mx[t] = a;
      __syncthreads();
    }
    const long long before = max(run_last, t ? mx[t - 1] : -1LL);        // the last non-zero position in front of chunk k
    const long long zeros = (long long)k * ESC_CHUNK - 1 - before;
    const uint32_t carry = zeros < 2 ? (uint32_t)zeros : 2u + (uint32_t)(zeros & 1);
    const uint32_t lead = carry == 0 ? r.lead[0] : carry == 1 ? r.lead[1] : carry == 2 ? r.lead[2] : r.lead[3];
    const uint32_t cnt = on ? r.local + lead : 0;
    if (ISOLATED && on && lead) atomicAdd(&J.seg_cnt[r.lead_seg], lead);
    sm[t] = cnt;
    __syncthreads();
    for (int o = 1; o < ESC_THREADS; o <<= 1) {                           // inclusive sum-scan
      const unsigned long long a = t >= o ? sm[t - o] : 0;
      __syncthreads();
      sm[t] += a;
      __syncthreads();
    }
    if (on) { J.recs[k].carry = carry; J.recs[k].out_off = (unsigned long long)k * ESC_CHUNK + run_sum + sm[t] - cnt; }
    const long long tile_last = mx[ESC_THREADS - 1]; const unsigned long long tile_sum = sm[ESC_THREADS - 1];
    __syncthreads();
    run_last = max(run_last, tile_last); run_sum += tile_sum;
  }
  // the final 03 behind a trailing 00 (write(), NALwrite.cpp:149-152)
  if (t == 0 && J.out_total) *J.out_total = (unsigned long long)J.total + run_sum + (J.total && run_last != (long long)J.total - 1 ? 1 : 0);
}

__global__ __launch_bounds__(ESC_THREADS) void k_esc_scatter(const EscJob* __restrict__ jobs) {
  __shared__ int part[4];
  __shared__ uint32_t spart[4];
  const EscJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks) return;
  const uint32_t chunk = blockIdx.x * (uint32_t)ESC_CHUNK;
  const EscRec R = J.recs[blockIdx.x];
  const int t = threadIdx.x, rel0 = t * ESC_LANE;
  uint8_t v[ESC_LANE];
  esc_load(J, chunk + rel0, v);
  const int n_valid = (int)min((uint32_t)ESC_LANE, J.total - min(J.total, chunk + rel0));
  int own = -1;
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) if (j < n_valid && v[j]) own = rel0 + j;
  const int prev = esc_block_max_before(own, part);
  // the zeros in front of the chunk's first byte as far as they matter: the carry class itself (2 and 3 stand for every larger even / odd number)
  const int carry = (int)R.carry;
  uint32_t flags = 0;
  int p = prev;
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) {
    if (j >= n_valid) continue;
    const int rel = rel0 + j;
    const int zeros = p < 0 ? rel + carry : rel - 1 - p;
    flags |= (uint32_t)esc_flag(zeros, v[j]) << j;
    if (v[j]) p = rel;
  }
  const uint32_t mine = __popc(flags);
  const uint32_t before = esc_block_sum_scan(mine, spart) - mine;
  unsigned long long at = R.out_off + (unsigned long long)rel0 + before;
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) {
    if (j >= n_valid) continue;
    if ((flags >> j) & 1u) { if (at < J.out_cap) J.out[at] = 3; at++; }
    if (at < J.out_cap) J.out[at] = v[j];
    at++;
    if (chunk + rel0 + j == J.total - 1 && v[j] == 0) { if (at < J.out_cap) J.out[at] = 3; }   // the final 03
  }
}

// ---- the other direction: emulation prevention removed (convertPayloadToRBSP, TLibDecoder/NALread.cpp:52-77) ----
// Byte i of the input is dropped exactly when it is 03 and the two bytes in front of it are 00 00: the sequential rule's counter is reset by the byte it drops, but that
// byte is not zero, so the counter at i is the number of zeros immediately in front of i in the INPUT and the predicate is local -- two bytes back, and one ahead for the
// second kind of violation.  No carry class, no max-scan:
//   k_une_count    per chunk the dropped bytes (and, per segment, into the segment's word by atomicAdd: TDecCAVLC.cpp:1343-1353), the violations
//   k_une_scan     one block per job: the dropped bytes in front of every chunk, the output's length
//   k_une_compact  the flags again, an exclusive prefix over the lanes, the kept bytes stored below the capacity only
struct UneJob {
  const uint8_t* in; uint32_t lookback, total;               // in[0 .. lookback): what only the predicate sees; then the segments, `total` bytes; positions count from their start
  const uint32_t* seg_end; uint32_t n_seg; uint32_t* seg_cnt;   // the segments' end positions (ascending, the last = total); per segment the bytes dropped inside it
  uint32_t* chunk_cnt; uint32_t n_chunks;                    // count: dropped in the chunk; after the scan: dropped in front of it
  uint8_t* out; unsigned long long out_cap; unsigned long long* out_total; uint32_t* violations;
};
__device__ static inline uint32_t une_segment_of(const UneJob& J, uint32_t pos) {
  uint32_t lo = 0, hi = J.n_seg - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (J.seg_end[mid] > pos) hi = mid; else lo = mid + 1; }
  return lo;
}
// the lane's 16 bytes from position `at` with the two in front and the one behind: w[k] = the byte at at - 2 + k; ff in front of the lookback, 00 behind the end.
// Returns the drop flags of the valid bytes; *viol: the violations among them.
__device__ static inline uint32_t une_flags(const UneJob& J, uint32_t at, int n_valid, uint8_t w[ESC_LANE + 3], uint32_t* viol) {
  const long long first = (long long)at - 2 + J.lookback;    // index into J.in of w[0]
  if (first >= 0 && at + ESC_LANE + 1 <= J.total) __builtin_memcpy(w, J.in + first, ESC_LANE + 3);
  else {
#pragma unroll
    for (int k = 0; k < ESC_LANE + 3; k++) { const long long i = first + k; w[k] = i < 0 ? 0xff : i < (long long)J.lookback + J.total ? J.in[i] : 0; }
  }
  uint32_t flags = 0, bad = 0;
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) {
    if (j >= n_valid) continue;
    const bool z2 = w[j] == 0 && w[j + 1] == 0;
    const uint8_t b = w[j + 2];
    const bool drop = z2 && b == 3;
    flags |= (uint32_t)drop << j;
    bad += (z2 && b <= 2) + (drop && w[j + 3] > 3);
  }
  if (viol) *viol = bad;
  return flags;
}

__global__ __launch_bounds__(ESC_THREADS) void k_une_count(const UneJob* __restrict__ jobs) {
  __shared__ uint32_t sums[4][2];
  const UneJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks) return;                                  // (uniform: the whole block)
  const uint32_t chunk = blockIdx.x * (uint32_t)ESC_CHUNK;
  const int t = threadIdx.x;
  const uint32_t at = chunk + (uint32_t)t * ESC_LANE;
  const int n_valid = (int)min((uint32_t)ESC_LANE, J.total - min(J.total, at));
  uint8_t w[ESC_LANE + 3];
  uint32_t bad = 0;
  const uint32_t flags = n_valid ? une_flags(J, at, n_valid, w, &bad) : 0u;
  const uint32_t last = min(J.total, chunk + (uint32_t)ESC_CHUNK) - 1;
  const uint32_t seg0 = une_segment_of(J, chunk);
  const bool one_segment = J.seg_end[seg0] > last;
  if (!one_segment && flags) {                                           // a chunk that holds a boundary: each dropped byte to the segment its position lies in
    uint32_t seg = une_segment_of(J, at), acc = 0;
#pragma unroll
    for (int j = 0; j < ESC_LANE; j++) {
      if (!((flags >> j) & 1u)) continue;
      while (at + j >= J.seg_end[seg]) { if (acc) atomicAdd(&J.seg_cnt[seg], acc); acc = 0; seg++; }
      acc++;
    }
    if (acc) atomicAdd(&J.seg_cnt[seg], acc);
  }
  uint32_t s2[2] = { (uint32_t)__popc(flags), bad };
#pragma unroll
  for (int k = 0; k < 2; k++) {
    uint32_t x = s2[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((t & 63) == 0) sums[t >> 6][k] = x;
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t cnt = sums[0][0] + sums[1][0] + sums[2][0] + sums[3][0], v = sums[0][1] + sums[1][1] + sums[2][1] + sums[3][1];
    J.chunk_cnt[blockIdx.x] = cnt;
    if (one_segment && cnt) atomicAdd(&J.seg_cnt[seg0], cnt);
    if (v) atomicAdd(J.violations, v);
  }
}

__global__ __launch_bounds__(ESC_THREADS) void k_une_scan(const UneJob* __restrict__ jobs) {
  __shared__ uint32_t part[4];
  const UneJob J = jobs[blockIdx.x];
  const int t = threadIdx.x;
  uint32_t run = 0;                                                      // dropped in front of the tile
  for (uint32_t base = 0; base < J.n_chunks; base += ESC_THREADS) {
    const uint32_t k = base + t;
    const uint32_t cnt = k < J.n_chunks ? J.chunk_cnt[k] : 0u;
    const uint32_t incl = esc_block_sum_scan(cnt, part);
    if (k < J.n_chunks) J.chunk_cnt[k] = run + incl - cnt;
    run += part[0] + part[1] + part[2] + part[3];
    __syncthreads();                                                     // (part is written again by the next tile)
  }
  if (t == 0) *J.out_total = (unsigned long long)J.total - run;
}

__global__ __launch_bounds__(ESC_THREADS) void k_une_compact(const UneJob* __restrict__ jobs) {
  __shared__ uint32_t part[4];
  const UneJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.n_chunks) return;
  const uint32_t chunk = blockIdx.x * (uint32_t)ESC_CHUNK;
  const uint32_t at = chunk + (uint32_t)threadIdx.x * ESC_LANE;
  const int n_valid = (int)min((uint32_t)ESC_LANE, J.total - min(J.total, at));
  uint8_t w[ESC_LANE + 3];
  const uint32_t flags = n_valid ? une_flags(J, at, n_valid, w, nullptr) : 0u;
  const uint32_t mine = __popc(flags);
  const uint32_t before = esc_block_sum_scan(mine, part) - mine;
  unsigned long long to = (unsigned long long)at - J.chunk_cnt[blockIdx.x] - before;
#pragma unroll
  for (int j = 0; j < ESC_LANE; j++) {
    if (j >= n_valid || ((flags >> j) & 1u)) continue;
    if (to < J.out_cap) J.out[to] = w[j + 2];
    to++;
  }
}

// sum over a plane of ((sample & 0xff) ^ m) [+ ((sample >> 8) ^ m) above 8 bit], m = (x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8) as an unsigned char
// (compChecksum, TComPicYuvMD5.cpp:141-164), modulo 2^32: exact in any order.  grid: (blocks, plane, picture); a lane takes four samples (8 bytes) at a time.
struct SumArgs { const int16_t* plane[3]; int w, h, pitch, pic_rows, deep; uint32_t* out; };
__global__ __launch_bounds__(256) void k_pic_checksum(SumArgs A) {
  __shared__ uint32_t part[4];
  const int comp = blockIdx.y, pic = blockIdx.z, sh = comp ? 1 : 0;
  const int w = A.w >> sh, h = A.h >> sh, pitch = A.pitch >> sh, quads = w >> 2;
  const int16_t* base = A.plane[comp] + (size_t)pic * (A.pic_rows >> sh) * pitch;
  uint32_t sum = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)quads * h; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / quads), x = (int)(i - (long long)y * quads) * 4;
    const uint2 q = *reinterpret_cast<const uint2*>(base + (size_t)y * pitch + x);
    const uint32_t s4[4] = { q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16 };
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t m = (((x + k) & 0xff) ^ (y & 0xff) ^ ((x + k) >> 8) ^ (y >> 8)) & 0xff;
      sum += (s4[k] & 0xff) ^ m;
      if (A.deep) sum += (s4[k] >> 8) ^ m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&A.out[pic * 3 + comp], part[0] + part[1] + part[2] + part[3]);
}

int pictures_of(const hop_ctx* c, int* ph) {
  *ph = c->sub_pitch ? c->sub_h : c->pic_h;
  return c->sub_pitch ? (c->pic_h - c->sub_h) / c->sub_pitch + 1 : 1;
}

// the checksum pass enqueued: d_sums = 3 words per picture (cleared here)
int launch_checksum(hop_ctx* c, uint32_t* d_sums) {
  int ph; const int n_pic = pictures_of(c, &ph);
  HIPCHK(c, hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * 3 * n_pic, c->stream));
  SumArgs A;
  for (int k = 0; k < 3; k++) A.plane[k] = c->rec[k];
  A.w = c->pic_w; A.h = ph; A.pitch = c->pic_w; A.pic_rows = c->sub_pitch ? c->sub_pitch : c->pic_h; A.deep = c->bd_y > 8; A.out = d_sums;
  const long long quads = (long long)(c->pic_w >> 2) * ph;
  const int blocks = (int)std::min<long long>((quads + 1023) / 1024, 1024);
  const int pr = hop_prof_begin(c, HOP_K_PICHASH, (uint64_t)c->pic_w * ph * 3 / 2 * n_pic);
  hipLaunchKernelGGL(k_pic_checksum, dim3(blocks, 3, n_pic), dim3(256), 0, c->stream, A);
  hop_prof_end(c, pr);
  HIPCHK(c, hipGetLastError());
  return HOP_OK;
}

void digest_of_sum(uint32_t s, uint8_t d[16]) { memset(d, 0, 16); d[0] = (uint8_t)(s >> 24); d[1] = (uint8_t)(s >> 16); d[2] = (uint8_t)(s >> 8); d[3] = (uint8_t)s; }

// MD5 of the resident planes: downloaded whole, hashed per picture on the host
int md5_pictures(hop_ctx* c, uint8_t (*digest)[16]) {
  int ph; const int n_pic = pictures_of(c, &ph);
  for (int comp = 0; comp < 3; comp++) {
    const int sh = comp ? 1 : 0, w = c->pic_w >> sh;
    std::vector<int16_t> plane((size_t)w * (c->pic_h >> sh));
    HIPCHK(c, hipMemcpyAsync(plane.data(), c->rec[comp], plane.size() * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < n_pic; k++) hop_strm_hash_plane(1, c->bd_y, plane.data() + (size_t)k * (c->sub_pitch >> sh) * w, w, ph >> sh, (size_t)w, digest[k * 3 + comp]);
  }
  return HOP_OK;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t chunks_of(size_t bytes) { return (uint32_t)((bytes + ESC_CHUNK - 1) / ESC_CHUNK); }

void launch_count_scan(hop_ctx* c, bool isolated, const EscJob* d_jobs, int n_jobs, uint32_t max_chunks) {
  if (isolated) {
    hipLaunchKernelGGL(k_esc_count<true>, dim3(max_chunks, n_jobs), dim3(ESC_THREADS), 0, c->stream, d_jobs);
    hipLaunchKernelGGL(k_esc_scan<true>, dim3(n_jobs), dim3(ESC_THREADS), 0, c->stream, d_jobs);
  } else {
    hipLaunchKernelGGL(k_esc_count<false>, dim3(max_chunks, n_jobs), dim3(ESC_THREADS), 0, c->stream, d_jobs);
    hipLaunchKernelGGL(k_esc_scan<false>, dim3(n_jobs), dim3(ESC_THREADS), 0, c->stream, d_jobs);
  }
}
}  // namespace

extern "C" int hop_picture_hash(hop_ctx* c, int method, uint8_t (*digest)[16]) {
  if (!c || !digest) return hop_set_err(c, HOP_ERR_ARG, "hop_picture_hash: bad argument");
  if (method != 1 && method != 3) return hop_set_err(c, HOP_ERR_ARG, "hop_picture_hash: method %d (1 MD5, 3 checksum; the CRC is not computed)", method);
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "hop_picture_hash: luma and chroma bit depths differ");
  if ((c->pic_w & 7) || (c->pic_h & 7) || (c->sub_h & 7)) return hop_set_err(c, HOP_ERR_ARG, "hop_picture_hash: the picture's dimensions are no multiples of 8");
  HIPCHK(c, hipSetDevice(c->device));
  if (method == 1) return md5_pictures(c, digest);
  int ph; const int n_pic = pictures_of(c, &ph);
  void* buf; int r = hop_scratch(c, sizeof(uint32_t) * 3 * n_pic, &buf); if (r) return r;
  r = launch_checksum(c, (uint32_t*)buf); if (r) return r;
  std::vector<uint32_t> sums(3 * (size_t)n_pic);
  HIPCHK(c, hipMemcpyAsync(sums.data(), buf, sizeof(uint32_t) * sums.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < sums.size(); i++) digest_of_sum(sums[i], digest[i]);
  return HOP_OK;
}

extern "C" int hop_rbsp_escape(hop_ctx* c, const uint8_t* rbsp, const uint32_t* segment_bytes, int32_t n_segments, uint8_t* out, size_t out_capacity, size_t* out_bytes,
                               uint32_t* segment_emulations) {
  if (!c || !rbsp || !segment_bytes || n_segments < 1 || !out_bytes || (!out && out_capacity)) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_escape: bad argument");
  std::vector<uint32_t> ends(n_segments);
  size_t total = 0;
  for (int i = 0; i < n_segments; i++) {
    if (!segment_bytes[i]) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_escape: segment %d is empty", i);
    total += segment_bytes[i];
    if (total > 0x7FFFFFFFu) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_escape: more than 2^31 - 1 bytes");
    ends[i] = (uint32_t)total;
  }
  const size_t dev_cap = std::min(out_capacity, total + total / 2 + 2);
  const uint32_t n_chunks = chunks_of(total);
  size_t end = 0;
  auto seg = [&](size_t bytes) { const size_t at = align256(end); end = at + bytes; return at; };
  const size_t o_data = seg(total + ESC_LANE), o_ends = seg(sizeof(uint32_t) * n_segments), o_cnt = seg(sizeof(uint32_t) * n_segments), o_recs = seg(sizeof(EscRec) * n_chunks),
               o_jobs = seg(sizeof(EscJob) * 2), o_total = seg(sizeof(unsigned long long)), o_out = seg(dev_cap + ESC_LANE);
  void* buf; int r = hop_scratch(c, end, &buf); if (r) return r;
  char* b = (char*)buf;
  HIPCHK(c, hipSetDevice(c->device));
  EscJob J[2];
  J[0].head = (const uint8_t*)(b + o_data); J[0].body = J[0].head; J[0].head_len = (uint32_t)total; J[0].total = (uint32_t)total;
  J[0].seg_end = (const uint32_t*)(b + o_ends); J[0].n_seg = (uint32_t)n_segments; J[0].seg_cnt = (uint32_t*)(b + o_cnt);
  J[0].recs = (EscRec*)(b + o_recs); J[0].n_chunks = n_chunks; J[0].out = (uint8_t*)(b + o_out); J[0].out_cap = dev_cap; J[0].out_total = nullptr;
  J[1] = J[0]; J[1].out_total = (unsigned long long*)(b + o_total);
  HIPCHK(c, hipMemcpyAsync(b + o_data, rbsp, total, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_ends, ends.data(), sizeof(uint32_t) * n_segments, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_cnt, 0, sizeof(uint32_t) * n_segments, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_jobs, J, sizeof(J), hipMemcpyHostToDevice, c->stream));
  const EscJob* dj = (const EscJob*)(b + o_jobs);
  const int pr = hop_prof_begin(c, HOP_K_ESCAPE, total);
  if (segment_emulations) launch_count_scan(c, true, dj, 1, n_chunks);   // the segments alone (the scan of job 0 stores no total)
  launch_count_scan(c, false, dj + 1, 1, n_chunks);
  hipLaunchKernelGGL(k_esc_scatter, dim3(n_chunks, 1), dim3(ESC_THREADS), 0, c->stream, dj + 1);
  hop_prof_end(c, pr);
  HIPCHK(c, hipGetLastError());
  unsigned long long need = 0;
  HIPCHK(c, hipMemcpyAsync(&need, b + o_total, sizeof(need), hipMemcpyDeviceToHost, c->stream));
  if (segment_emulations) HIPCHK(c, hipMemcpyAsync(segment_emulations, b + o_cnt, sizeof(uint32_t) * n_segments, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out_bytes = (size_t)need;
  if (need > out_capacity) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_escape: the escaped bytes take %llu bytes, out_capacity is %zu", need, out_capacity);
  if (need > dev_cap) return hop_set_err(c, HOP_ERR_DEVICE, "hop_rbsp_escape: %llu bytes from %zu", need, total);
  HIPCHK(c, hipMemcpy(out, b + o_out, (size_t)need, hipMemcpyDeviceToHost));
  return HOP_OK;
}

extern "C" int hop_access_unit_write(hop_ctx* c, const hop_stream_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao, uint8_t* out,
                                     size_t out_capacity, size_t* au_bytes) {
  if (!c || !p || !parts || !au_bytes || (!out && out_capacity)) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_write: bad argument");
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_write: a sharded context writes no stream");
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_write: luma and chroma bit depths differ");
  int ph; const int n_pic = pictures_of(c, &ph);
  char err[256];
  int r = hop_strm_check(c->pic_w, ph, c->bd_y, p, err, sizeof(err));
  if (r) return hop_set_err(c, r, "%s", err);
  const int hctu = (ph + 63) / 64, n_sub = p->slice.wpp ? hctu : 1, n_seg = n_pic * n_sub;
  // what every access unit carries besides its slice NAL unit, and the slice NAL unit's header at its longest (a few bytes and up to four per entry point)
  std::vector<uint8_t> sets;
  if (p->parameter_sets) hop_strm_parameter_sets(c->pic_w, ph, c->bd_y, p, sets);
  const size_t start_code = p->parameter_sets ? 3 : 4, head_max = 32 + 4 * (size_t)n_sub;
  // the slice data, left on the device; behind it in the same allocation everything the escape needs: its size follows from the capacity, which bounds the slice data
  // (never more than the slice-data writer's own bound: 48 KiB per CTU)
  const size_t sd_cap = std::min<size_t>(out_capacity, (size_t)n_pic * ((c->pic_w + 63) / 64) * hctu * 49152 + 256 * (size_t)n_seg);
  const size_t in_max = sd_cap + (size_t)n_pic * head_max, out_max = in_max + in_max / 2 + 2 * (size_t)n_pic + 32 * (size_t)n_pic;
  const size_t chunks_max = in_max / ESC_CHUNK + 2 * (size_t)n_pic + 1;
  size_t end = 0;
  auto seg = [&](size_t bytes) { const size_t at = align256(end); end = at + bytes; return at; };
  const size_t o_heads = seg(n_pic * align256(head_max) + ESC_LANE), o_ends = seg(sizeof(uint32_t) * n_seg), o_cnt = seg(sizeof(uint32_t) * n_seg),
               o_recs = seg(sizeof(EscRec) * chunks_max), o_jobs = seg(sizeof(EscJob) * (n_pic + 1)), o_totals = seg(sizeof(unsigned long long) * n_pic),
               o_sums = seg(sizeof(uint32_t) * 3 * n_pic), o_out = seg(out_max + ESC_LANE);
  std::vector<uint32_t> sub(n_seg);
  int32_t got = -1;
  const uint8_t* d_packed = nullptr; uint8_t* d_res = nullptr;
  const int32_t* pic_qp = hop_picture_qps(c);                             // hop_ctx_set_picture_qps: picture k's slice data and slice_qp_delta at its own QP; the parameter sets carry none
  r = hop_ent_write_device(c, &p->slice, parts, levels, sao, nullptr, sd_cap, sub.data(), &got, end, &d_packed, &d_res, pic_qp);
  if (r == HOP_ERR_ARG && got >= 0 && (size_t)got > sd_cap) {
    // the slice data alone outgrows the capacity: the size needed comes from a run into a buffer of our own that holds it
    size_t sd = 0; for (int i = 0; i < n_seg; i++) sd += sub[i];
    std::vector<uint8_t> tmp(sd + sd / 2 + (size_t)n_pic * (head_max + sets.size() + 128));
    std::vector<size_t> each(n_pic);
    r = hop_access_unit_write(c, p, parts, levels, sao, tmp.data(), tmp.size(), each.data());
    if (r) return r;
    size_t need = 0; for (int k = 0; k < n_pic; k++) need += each[k];
    au_bytes[0] = need;
    return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_write: the access units take %zu bytes, out_capacity is %zu", need, out_capacity);
  }
  if (r) return r;
  char* b = (char*)d_res;
  // 1. every substream's emulation count alone: one job over the packed substreams
  std::vector<uint32_t> ends(n_seg);
  size_t sd_total = 0;
  for (int i = 0; i < n_seg; i++) { sd_total += sub[i]; ends[i] = (uint32_t)sd_total; }
  std::vector<EscJob> J(n_pic + 1);
  EscJob& iso = J[n_pic];
  iso.head = d_packed; iso.body = d_packed; iso.head_len = (uint32_t)sd_total; iso.total = (uint32_t)sd_total;
  iso.seg_end = (const uint32_t*)(b + o_ends); iso.n_seg = (uint32_t)n_seg; iso.seg_cnt = (uint32_t*)(b + o_cnt);
  iso.recs = (EscRec*)(b + o_recs); iso.n_chunks = chunks_of(sd_total); iso.out = nullptr; iso.out_cap = 0; iso.out_total = nullptr;
  HIPCHK(c, hipMemcpyAsync(b + o_ends, ends.data(), sizeof(uint32_t) * n_seg, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_cnt, 0, sizeof(uint32_t) * n_seg, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_jobs + sizeof(EscJob) * n_pic, &iso, sizeof(EscJob), hipMemcpyHostToDevice, c->stream));
  const int pr0 = hop_prof_begin(c, HOP_K_ESCAPE, sd_total);
  launch_count_scan(c, true, (const EscJob*)(b + o_jobs) + n_pic, 1, iso.n_chunks);
  hop_prof_end(c, pr0);
  HIPCHK(c, hipGetLastError());
  if (p->hash == 3) { r = launch_checksum(c, (uint32_t*)(b + o_sums)); if (r) return r; }
  std::vector<uint32_t> emul(n_seg), sums(3 * (size_t)n_pic);
  HIPCHK(c, hipMemcpyAsync(emul.data(), b + o_cnt, sizeof(uint32_t) * n_seg, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // 2. NAL header and slice header of every picture, uploaded; a job per picture over header + substreams
  std::vector<uint8_t> heads((size_t)n_pic * align256(head_max));
  uint32_t max_chunks = 0; size_t out_at = 0, body_at = 0, rec_at = 0;
  for (int k = 0; k < n_pic; k++) {
    std::vector<uint8_t> h;
    hop_stream_params pk = *p;
    if (pic_qp) pk.slice.qp = pic_qp[k];
    hop_strm_slice_header(c->pic_w, ph, &pk, &sub[(size_t)k * n_sub], &emul[(size_t)k * n_sub], n_sub, h);
    if (h.size() > head_max) return hop_set_err(c, HOP_ERR_DEVICE, "hop_access_unit_write: slice header of %zu bytes", h.size());
    memcpy(&heads[(size_t)k * align256(head_max)], h.data(), h.size());
    size_t body = 0; for (int s = 0; s < n_sub; s++) body += sub[(size_t)k * n_sub + s];
    EscJob& j = J[k];
    j.head = (const uint8_t*)(b + o_heads) + (size_t)k * align256(head_max); j.head_len = (uint32_t)h.size();
    j.body = d_packed + body_at; j.total = (uint32_t)(h.size() + body);
    j.seg_end = nullptr; j.n_seg = 1; j.seg_cnt = nullptr;
    j.n_chunks = chunks_of(j.total); j.recs = (EscRec*)(b + o_recs) + rec_at;
    j.out = (uint8_t*)(b + o_out) + out_at; j.out_cap = (size_t)j.total + j.total / 2 + 2; j.out_total = (unsigned long long*)(b + o_totals) + k;
    max_chunks = std::max(max_chunks, j.n_chunks);
    body_at += body; rec_at += j.n_chunks; out_at += (j.out_cap + 15) & ~(size_t)15;
  }
  if (rec_at > chunks_max || out_at > out_max) return hop_set_err(c, HOP_ERR_DEVICE, "hop_access_unit_write: work area of %zu chunks, %zu bytes outgrown", chunks_max, out_max);
  HIPCHK(c, hipMemcpyAsync(b + o_heads, heads.data(), heads.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_jobs, J.data(), sizeof(EscJob) * n_pic, hipMemcpyHostToDevice, c->stream));
  const int pr1 = hop_prof_begin(c, HOP_K_ESCAPE, sd_total + (size_t)n_pic * head_max);
  launch_count_scan(c, false, (const EscJob*)(b + o_jobs), n_pic, max_chunks);
  hipLaunchKernelGGL(k_esc_scatter, dim3(max_chunks, n_pic), dim3(ESC_THREADS), 0, c->stream, (const EscJob*)(b + o_jobs));
  hop_prof_end(c, pr1);
  HIPCHK(c, hipGetLastError());
  std::vector<unsigned long long> nal(n_pic);
  HIPCHK(c, hipMemcpyAsync(nal.data(), b + o_totals, sizeof(unsigned long long) * n_pic, hipMemcpyDeviceToHost, c->stream));
  if (p->hash == 3) HIPCHK(c, hipMemcpyAsync(sums.data(), b + o_sums, sizeof(uint32_t) * sums.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // 3. the hash SEI of every picture
  std::vector<std::vector<uint8_t>> sei(n_pic);
  if (p->hash) {
    std::vector<uint8_t> digest((size_t)n_pic * 3 * 16);
    uint8_t (*d)[16] = (uint8_t (*)[16])digest.data();
    if (p->hash == 3) for (size_t i = 0; i < sums.size(); i++) digest_of_sum(sums[i], d[i]);
    else { r = md5_pictures(c, d); if (r) return r; }
    for (int k = 0; k < n_pic; k++) hop_strm_sei(p->hash, (const uint8_t (*)[16])(d + 3 * k), sei[k]);
  }
  // 4. the access units: sizes first, then the bytes -- each finished NAL unit straight from the device into its place
  size_t need = 0;
  for (int k = 0; k < n_pic; k++) {
    if (nal[k] > J[k].out_cap) return hop_set_err(c, HOP_ERR_DEVICE, "hop_access_unit_write: picture %d: %llu escaped bytes from %u", k, nal[k], J[k].total);
    need += sets.size() + start_code + (size_t)nal[k] + sei[k].size();
  }
  if (need > out_capacity) {
    au_bytes[0] = need;
    return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_write: the access units take %zu bytes, out_capacity is %zu", need, out_capacity);
  }
  size_t at = 0;
  for (int k = 0; k < n_pic; k++) {
    const size_t from = at;
    if (!sets.empty()) { memcpy(out + at, sets.data(), sets.size()); at += sets.size(); }
    if (start_code == 4) out[at++] = 0;
    out[at++] = 0; out[at++] = 0; out[at++] = 1;
    HIPCHK(c, hipMemcpyAsync(out + at, J[k].out, (size_t)nal[k], hipMemcpyDeviceToHost, c->stream));
    at += (size_t)nal[k];
    if (!sei[k].empty()) { memcpy(out + at, sei[k].data(), sei[k].size()); at += sei[k].size(); }
    au_bytes[k] = at - from;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HOP_OK;
}

// ---- the stream read back ----
namespace {
// the work area of one unescape job behind `front` bytes of the caller's
struct UneArea { size_t o_ends, o_cnt, o_chunks, o_job, o_total, o_viol, o_out, end; uint32_t n_chunks; size_t dev_cap; };
UneArea une_area(size_t front, size_t total, int n_seg, size_t out_capacity) {
  UneArea A;
  size_t end = front;
  auto seg = [&](size_t bytes) { const size_t at = align256(end); end = at + bytes; return at; };
  A.n_chunks = chunks_of(total); A.dev_cap = std::min(out_capacity, total);
  A.o_ends = seg(sizeof(uint32_t) * n_seg); A.o_cnt = seg(sizeof(uint32_t) * n_seg); A.o_chunks = seg(sizeof(uint32_t) * A.n_chunks); A.o_job = seg(sizeof(UneJob));
  A.o_total = seg(sizeof(unsigned long long)); A.o_viol = seg(sizeof(uint32_t)); A.o_out = seg(A.dev_cap + ESC_LANE);
  A.end = end;
  return A;
}
// the three launches over d_in (lookback bytes, then the segments) enqueued, and what the host needs of their results brought back: the output's length, per segment
// its RBSP bytes, the violations.  The RBSP stays at b + A.o_out.
int une_run(hop_ctx* c, char* b, const UneArea& A, const uint8_t* d_in, int lookback, const uint32_t* segment_bytes, int n_seg, size_t total, unsigned long long* need,
            uint32_t* rbsp_bytes, uint32_t* violations) {
  std::vector<uint32_t> ends(n_seg);
  { size_t at = 0; for (int i = 0; i < n_seg; i++) { at += segment_bytes[i]; ends[i] = (uint32_t)at; } }
  UneJob J;
  J.in = d_in; J.lookback = (uint32_t)lookback; J.total = (uint32_t)total;
  J.seg_end = (const uint32_t*)(b + A.o_ends); J.n_seg = (uint32_t)n_seg; J.seg_cnt = (uint32_t*)(b + A.o_cnt);
  J.chunk_cnt = (uint32_t*)(b + A.o_chunks); J.n_chunks = A.n_chunks;
  J.out = (uint8_t*)(b + A.o_out); J.out_cap = A.dev_cap; J.out_total = (unsigned long long*)(b + A.o_total); J.violations = (uint32_t*)(b + A.o_viol);
  HIPCHK(c, hipMemcpyAsync(b + A.o_ends, ends.data(), sizeof(uint32_t) * n_seg, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(b + A.o_cnt, 0, sizeof(uint32_t) * n_seg, c->stream));
  HIPCHK(c, hipMemsetAsync(b + A.o_viol, 0, sizeof(uint32_t), c->stream));
  HIPCHK(c, hipMemcpyAsync(b + A.o_job, &J, sizeof(J), hipMemcpyHostToDevice, c->stream));
  const UneJob* dj = (const UneJob*)(b + A.o_job);
  const int pr = hop_prof_begin(c, HOP_K_UNESCAPE, total);
  hipLaunchKernelGGL(k_une_count, dim3(A.n_chunks, 1), dim3(ESC_THREADS), 0, c->stream, dj);
  hipLaunchKernelGGL(k_une_scan, dim3(1), dim3(ESC_THREADS), 0, c->stream, dj);
  hipLaunchKernelGGL(k_une_compact, dim3(A.n_chunks, 1), dim3(ESC_THREADS), 0, c->stream, dj);
  hop_prof_end(c, pr);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> cnt(n_seg);
  uint32_t viol = 0;
  HIPCHK(c, hipMemcpyAsync(need, b + A.o_total, sizeof(*need), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cnt.data(), b + A.o_cnt, sizeof(uint32_t) * n_seg, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&viol, b + A.o_viol, sizeof(viol), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long dropped = 0;
  for (int i = 0; i < n_seg; i++) {
    if (cnt[i] > segment_bytes[i]) return hop_set_err(c, HOP_ERR_DEVICE, "hop_rbsp_unescape: segment %d: %u of %u bytes dropped", i, cnt[i], segment_bytes[i]);
    dropped += cnt[i];
    if (rbsp_bytes) rbsp_bytes[i] = segment_bytes[i] - cnt[i];
  }
  if (*need + dropped != total) return hop_set_err(c, HOP_ERR_DEVICE, "hop_rbsp_unescape: %llu bytes kept and %llu dropped of %zu", *need, dropped, total);
  if (violations) *violations = viol;
  return HOP_OK;
}

// what hop_access_unit_read and hop_access_unit_decode share: the host pass over the syntax, the VCL unit's payload uploaded, the three launches.  Afterwards the
// slice data's RBSP (*total bytes, sizes[] per substream) lies at *d_rbsp inside the first *front bytes of the scratch area, which was sized front + tail(front).
template <typename Tail>
int au_unescape(hop_ctx* c, const char* who, const uint8_t* au, size_t au_bytes, const hop_stream_info* active, int max_substreams, Tail tail, hop_strm_au& a,
                std::vector<uint32_t>& sizes, size_t* total, const uint8_t** d_rbsp, size_t* front) {
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "%s: a sharded context reads no stream", who);
  if (c->sub_pitch || c->sub_h) return hop_set_err(c, HOP_ERR_ARG, "%s: a stacked context reads no stream (one picture per context)", who);
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "%s: luma and chroma bit depths differ", who);
  const int dims[3] = { c->pic_w, c->pic_h, c->bd_y };
  char err[256];
  int r = hop_strm_read_syntax(au, au_bytes, active, dims, max_substreams, &a, err, sizeof(err));
  if (r) return hop_set_err(c, r, "%s", err);
  const int n_sub = (int)a.seg.size(), back = std::min(2, (int)a.info.header_bytes);
  const size_t payload = a.nal_len - (size_t)a.info.header_bytes;
  const size_t o_in = 0, in_bytes = (size_t)back + payload;
  const UneArea A = une_area(o_in + in_bytes + ESC_LANE, payload, n_sub, payload);
  *front = align256(A.end);
  void* buf; r = hop_scratch(c, *front + tail(*front), &buf); if (r) return r;
  char* b = (char*)buf;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b + o_in, au + a.nal_at + a.info.header_bytes - back, in_bytes, hipMemcpyHostToDevice, c->stream));
  unsigned long long need = 0; uint32_t viol = 0;
  sizes.assign(n_sub, 0);
  r = une_run(c, b, A, (const uint8_t*)(b + o_in), back, a.seg.data(), n_sub, payload, &need, sizes.data(), &viol);
  if (r) return r;
  r = hop_strm_read_sizes(sizes.data(), n_sub, viol, err, sizeof(err));
  if (r) return hop_set_err(c, r, "%s", err);
  *total = (size_t)need; *d_rbsp = (const uint8_t*)(b + A.o_out);
  return HOP_OK;
}
}  // namespace

extern "C" int hop_rbsp_unescape(hop_ctx* c, const uint8_t* escaped, const uint32_t* segment_bytes, int32_t n_segments, int32_t lookback, uint8_t* out, size_t out_capacity,
                                 size_t* out_bytes, uint32_t* segment_rbsp_bytes, uint32_t* violations) {
  if (!c || !escaped || !segment_bytes || n_segments < 1 || lookback < 0 || lookback > 2 || !out_bytes || (!out && out_capacity))
    return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_unescape: bad argument");
  size_t total = 0;
  for (int i = 0; i < n_segments; i++) {
    if (!segment_bytes[i]) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_unescape: segment %d is empty", i);
    total += segment_bytes[i];
    if (total > 0x7FFFFFFFu) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_unescape: more than 2^31 - 1 bytes");
  }
  const size_t in_bytes = (size_t)lookback + total;
  const UneArea A = une_area(in_bytes + ESC_LANE, total, n_segments, out_capacity);
  void* buf; int r = hop_scratch(c, A.end, &buf); if (r) return r;
  char* b = (char*)buf;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b, escaped, in_bytes, hipMemcpyHostToDevice, c->stream));
  unsigned long long need = 0;
  r = une_run(c, b, A, (const uint8_t*)b, lookback, segment_bytes, n_segments, total, &need, segment_rbsp_bytes, violations);
  if (r) return r;
  *out_bytes = (size_t)need;
  if (need > out_capacity) return hop_set_err(c, HOP_ERR_ARG, "hop_rbsp_unescape: the RBSP takes %llu bytes, out_capacity is %zu", need, out_capacity);
  if (need) HIPCHK(c, hipMemcpy(out, b + A.o_out, (size_t)need, hipMemcpyDeviceToHost));
  return HOP_OK;
}

extern "C" int hop_access_unit_read(hop_ctx* c, const uint8_t* au, size_t au_bytes, const hop_stream_info* active, hop_stream_info* info, uint8_t* data, size_t data_capacity,
                                    size_t* data_bytes, uint32_t* substream_bytes, int32_t max_substreams, uint8_t (*digest)[16]) {
  if (!c || !au || !info || !data_bytes || !substream_bytes || !digest || (!data && data_capacity)) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_read: bad argument");
  hop_strm_au a; std::vector<uint32_t> sizes; size_t total = 0, front = 0; const uint8_t* d_rbsp = nullptr;
  int r = au_unescape(c, "hop_access_unit_read", au, au_bytes, active, max_substreams, [](size_t) { return (size_t)0; }, a, sizes, &total, &d_rbsp, &front);
  if (r) return r;
  memcpy(substream_bytes, sizes.data(), sizeof(uint32_t) * sizes.size());
  *data_bytes = total; *info = a.info;
  memcpy(digest, a.digest, sizeof(a.digest));
  if (total > data_capacity) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_read: the slice data takes %zu bytes, data_capacity is %zu", total, data_capacity);
  HIPCHK(c, hipMemcpy(data, d_rbsp, total, hipMemcpyDeviceToHost));
  return HOP_OK;
}

extern "C" int hop_access_unit_decode(hop_ctx* c, const uint8_t* au, size_t au_bytes, const hop_stream_info* active, hop_stream_info* info, int32_t hash_match[3],
                                      hop_cu_part* parts, int32_t* levels, hop_sao_param* sao_coded) {
  if (!c || !au || !info || !hash_match) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_decode: bad argument");
  const int wctu = (c->pic_w + 63) / 64, hctu = (c->pic_h + 63) / 64, n_ctu = wctu * hctu;
  hop_strm_au a; std::vector<uint32_t> sizes; size_t total = 0, front = 0; const uint8_t* d_rbsp = nullptr;
  // the parser's work area goes behind the unescape's in one allocation, so that the RBSP stays where the compact kernel put it
  int r = au_unescape(c, "hop_access_unit_decode", au, au_bytes, active, hctu, [&](size_t) { return hop_parse_work_bytes(c, 0, hctu); }, a, sizes, &total, &d_rbsp, &front);
  if (r) return r;
  const hop_slice_data_params& sl = a.info.params.slice;
  const bool sao_on = sl.sao_luma || sl.sao_chroma;
  std::vector<hop_cu_part> own_parts; std::vector<int32_t> own_levels; std::vector<hop_sao_param> own_sao;
  if (!parts) { own_parts.resize((size_t)n_ctu * 256); parts = own_parts.data(); }
  if (!levels) { own_levels.resize((size_t)n_ctu * 6144); levels = own_levels.data(); }
  if (sao_on && !sao_coded) { own_sao.resize((size_t)n_ctu * 3); sao_coded = own_sao.data(); }
  // the stream's own QP all the way down: this entry does not read the context's table (hop_ctx_set_picture_qps).  (A stacked context is refused by hop_decode_frame below.)
  const int32_t own_qp[1] = { sl.qp }; const int32_t* au_qp = (c->sub_pitch || c->sub_h) ? nullptr : own_qp;
  r = hop_parse_device(c, &sl, nullptr, d_rbsp, sizes.data(), (int32_t)sizes.size(), parts, levels, sao_on ? sao_coded : nullptr, front, au_qp);
  if (r) return r;
  hop_dec_params dp; dp.qp = sl.qp; dp.cb_qp_offset = 0; dp.cr_qp_offset = 0; dp.plain_intra = sl.plain_intra; dp.schedule = 0;
  r = hop_decode_frame(c, &dp, parts, levels); if (r) return r;
  hop_deblock_params db; db.qp = sl.qp; db.beta_offset_div2 = 0; db.tc_offset_div2 = 0; db.cb_qp_offset = 0; db.cr_qp_offset = 0; db.disable = 0;
  r = hop_dbk_device(c, &db, parts, au_qp); if (r) return r;
  if (sao_on) {
    std::vector<hop_sao_param> recon((size_t)n_ctu * 3);
    if (hop_sao_reconstruct_params(n_ctu, wctu, c->bd_y, sao_coded, recon.data())) return hop_set_err(c, HOP_ERR_ARG, "hop_access_unit_decode: the coded SAO parameters name a merge candidate that is not there");
    r = hop_sao_apply(c, recon.data()); if (r) return r;
  }
  hash_match[0] = hash_match[1] = hash_match[2] = -1;
  if (a.info.params.hash == 1 || a.info.params.hash == 3) {
    uint8_t got[3][16];
    r = hop_picture_hash(c, a.info.params.hash, got); if (r) return r;
    for (int k = 0; k < 3; k++) hash_match[k] = !memcmp(got[k], a.digest[k], 16);
  }
  *info = a.info;
  return HOP_OK;
}

// ---- n access units into the n pictures of a stacked context ----
// One upload of the stream, one set of unescape launches with the access units as the grid's y dimension, one parse, one decode, one pass of each loop filter: what
// hop_access_unit_decode does per picture, done once for the stack.  The scratch area is laid out after the host pass over every access unit's syntax, when all sizes are
// known, and does not move afterwards: the stream and the unescape's records and outputs first (`front` bytes), the parser's work area behind them, then the decoder's
// CTU order.  The parser reads each substream where the compact kernel left it (its device offset) and k_dec_ctu reads parts and levels where the parser left them.
namespace {
const char* strip_prefix(const char* s, const char* prefix) { const size_t n = strlen(prefix); return strncmp(s, prefix, n) ? s : s + n; }

// the first field of the slice parameters, the QP aside (every picture of a stack is parsed, decoded and deblocked at its own), in which b differs from a, or NULL
const char* slice_params_differ(const hop_slice_data_params& a, const hop_slice_data_params& b, int* va, int* vb) {
  const struct { const char* name; int32_t x, y; } f[6] = { { "slice_type", a.slice_type, b.slice_type }, { "wpp", a.wpp, b.wpp },
    { "plain_intra", a.plain_intra, b.plain_intra }, { "sao_luma", a.sao_luma, b.sao_luma }, { "sao_chroma", a.sao_chroma, b.sao_chroma }, { "mi_size", a.mi_size, b.mi_size } };
  for (int k = 0; k < 6; k++) if (f[k].x != f[k].y) { *va = f[k].x; *vb = f[k].y; return f[k].name; }
  return nullptr;
}
}  // namespace

extern "C" int hop_access_units_decode(hop_ctx* c, const uint8_t* stream, const size_t* au_bytes, int32_t n_au, const hop_stream_info* active, hop_stream_info* info,
                                       int32_t (*hash_match)[3], hop_cu_part* parts, int32_t* levels, hop_sao_param* sao_coded) {
  static const char who[] = "hop_access_units_decode";
  if (!c || !stream || !au_bytes || n_au < 1 || !info || !hash_match) return hop_set_err(c, HOP_ERR_ARG, "%s: bad argument", who);
  if (c->shard_world > 1) return hop_set_err(c, HOP_ERR_ARG, "%s: a sharded context reads no stream", who);
  if (c->bd_y != c->bd_c) return hop_set_err(c, HOP_ERR_ARG, "%s: luma and chroma bit depths differ", who);
  int ph; const int n_pic = pictures_of(c, &ph);
  if (n_au != n_pic) return hop_set_err(c, HOP_ERR_ARG, "%s: %d access units, the context holds %d picture%s (a shorter tail of a sequence takes a context of its own)", who, n_au, n_pic, n_pic > 1 ? "s" : "");
  const int wctu = (c->pic_w + 63) / 64, hctu = (ph + 63) / 64, n_ctu = wctu * hctu;
  const size_t n = (size_t)n_ctu * n_pic;
  // 1. the host pass over every access unit's syntax: access unit k against the nearest earlier one of this call that carried parameter sets, else against `active`
  std::vector<hop_strm_au> a(n_au);
  std::vector<size_t> au_at(n_au);
  const int dims[3] = { c->pic_w, ph, c->bd_y };
  char err[256];
  size_t stream_bytes = 0, payload_total = 0;
  {
    const hop_stream_info* act = active;
    for (int k = 0; k < n_au; k++) {
      au_at[k] = stream_bytes;
      const int r = hop_strm_read_syntax(stream + stream_bytes, au_bytes[k], act, dims, hctu, &a[k], err, sizeof(err));
      if (r) return hop_set_err(c, r, "%s: access unit %d: %s", who, k, strip_prefix(err, "hop_access_unit_read: "));
      int v0 = 0, vk = 0;
      if (const char* field = slice_params_differ(a[0].info.params.slice, a[k].info.params.slice, &v0, &vk))
        return hop_set_err(c, HOP_ERR_ARG, "%s: access unit %d: %s is %d, access unit 0 has %d (one parse serves all pictures of a stack)", who, k, field, vk, v0);
      if (a[k].info.params.parameter_sets) act = &a[k].info;
      if (stream_bytes + au_bytes[k] < stream_bytes) return hop_set_err(c, HOP_ERR_ARG, "%s: the access units' sizes overflow", who);
      stream_bytes += au_bytes[k];
      payload_total += a[k].nal_len - (size_t)a[k].info.header_bytes;
    }
  }
  const hop_slice_data_params sl = a[0].info.params.slice;
  const bool sao_on = sl.sao_luma || sl.sao_chroma;
  const int n_sub = (int)a[0].seg.size(), n_seg = n_sub * n_au;       // (every access unit has the picture's CTU rows, or 1: the reader checked it)
  for (int k = 1; k < n_au; k++) if ((int)a[k].seg.size() != n_sub) return hop_set_err(c, HOP_ERR_ARG, "%s: access unit %d: %zu substreams, access unit 0 has %d", who, k, a[k].seg.size(), n_sub);
  // the scratch area, sized once
  std::vector<size_t> o_out(n_au), chunk_at(n_au);
  size_t end = 0, chunks_total = 0; uint32_t max_chunks = 0;
  auto seg = [&](size_t bytes) { const size_t at = align256(end); end = at + bytes; return at; };
  for (int k = 0; k < n_au; k++) { chunk_at[k] = chunks_total; const uint32_t nc = chunks_of(a[k].nal_len - (size_t)a[k].info.header_bytes); chunks_total += nc; max_chunks = std::max(max_chunks, nc); }
  const size_t o_in = seg(stream_bytes + ESC_LANE + 3), o_ends = seg(sizeof(uint32_t) * n_seg), o_cnt = seg(sizeof(uint32_t) * n_seg), o_chunks = seg(sizeof(uint32_t) * chunks_total),
               o_jobs = seg(sizeof(UneJob) * n_au), o_totals = seg(sizeof(unsigned long long) * n_au), o_viol = seg(sizeof(uint32_t) * n_au);
  for (int k = 0; k < n_au; k++) o_out[k] = seg(a[k].nal_len - (size_t)a[k].info.header_bytes + ESC_LANE);
  const size_t front = align256(end), o_order = align256(front + hop_parse_work_bytes(c, 0, n_sub)), total = o_order + sizeof(int32_t) * (n + 3 * (size_t)n_pic);   // (the CTU order and, behind it, the pictures' scaled QPs)
  void* buf; int r = hop_scratch(c, total, &buf); if (r) return r;
  char* b = (char*)buf;
  HIPCHK(c, hipSetDevice(c->device));
  // 2. emulation prevention removed from every access unit's slice data; the RBSP stays on the device
  std::vector<uint32_t> ends(n_seg);
  std::vector<UneJob> J(n_au);
  for (int k = 0; k < n_au; k++) {
    const int back = std::min(2, (int)a[k].info.header_bytes);
    const size_t payload = a[k].nal_len - (size_t)a[k].info.header_bytes;
    size_t at = 0;
    for (int i = 0; i < n_sub; i++) { at += a[k].seg[i]; ends[(size_t)k * n_sub + i] = (uint32_t)at; }
    UneJob& j = J[k];
    j.in = (const uint8_t*)(b + o_in) + au_at[k] + a[k].nal_at + a[k].info.header_bytes - back; j.lookback = (uint32_t)back; j.total = (uint32_t)payload;
    j.seg_end = (const uint32_t*)(b + o_ends) + (size_t)k * n_sub; j.n_seg = (uint32_t)n_sub; j.seg_cnt = (uint32_t*)(b + o_cnt) + (size_t)k * n_sub;
    j.chunk_cnt = (uint32_t*)(b + o_chunks) + chunk_at[k]; j.n_chunks = chunks_of(payload);
    j.out = (uint8_t*)(b + o_out[k]); j.out_cap = payload; j.out_total = (unsigned long long*)(b + o_totals) + k; j.violations = (uint32_t*)(b + o_viol) + k;
  }
  HIPCHK(c, hipMemcpyAsync(b + o_in, stream, stream_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_ends, ends.data(), sizeof(uint32_t) * n_seg, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_cnt, 0, sizeof(uint32_t) * n_seg, c->stream));
  HIPCHK(c, hipMemsetAsync(b + o_viol, 0, sizeof(uint32_t) * n_au, c->stream));
  HIPCHK(c, hipMemcpyAsync(b + o_jobs, J.data(), sizeof(UneJob) * n_au, hipMemcpyHostToDevice, c->stream));
  {
    const UneJob* dj = (const UneJob*)(b + o_jobs);
    const int pr = hop_prof_begin(c, HOP_K_UNESCAPE, payload_total);
    hipLaunchKernelGGL(k_une_count, dim3(max_chunks, n_au), dim3(ESC_THREADS), 0, c->stream, dj);
    hipLaunchKernelGGL(k_une_scan, dim3(n_au), dim3(ESC_THREADS), 0, c->stream, dj);
    hipLaunchKernelGGL(k_une_compact, dim3(max_chunks, n_au), dim3(ESC_THREADS), 0, c->stream, dj);
    hop_prof_end(c, pr);
    HIPCHK(c, hipGetLastError());
  }
  std::vector<unsigned long long> need(n_au);
  std::vector<uint32_t> cnt(n_seg), viol(n_au), sizes(n_seg);
  std::vector<unsigned long long> offs(n_seg);
  HIPCHK(c, hipMemcpyAsync(need.data(), b + o_totals, sizeof(unsigned long long) * n_au, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cnt.data(), b + o_cnt, sizeof(uint32_t) * n_seg, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(viol.data(), b + o_viol, sizeof(uint32_t) * n_au, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < n_au; k++) {
    unsigned long long dropped = 0, at = o_out[k];
    for (int i = 0; i < n_sub; i++) {
      const size_t s = (size_t)k * n_sub + i;
      if (cnt[s] > a[k].seg[i]) return hop_set_err(c, HOP_ERR_DEVICE, "%s: access unit %d, substream %d: %u of %u bytes dropped", who, k, i, cnt[s], a[k].seg[i]);
      dropped += cnt[s]; sizes[s] = a[k].seg[i] - cnt[s]; offs[s] = at; at += sizes[s];
    }
    if (need[k] + dropped != J[k].total) return hop_set_err(c, HOP_ERR_DEVICE, "%s: access unit %d: %llu bytes kept and %llu dropped of %u", who, k, need[k], dropped, J[k].total);
    r = hop_strm_read_sizes(&sizes[(size_t)k * n_sub], n_sub, viol[k], err, sizeof(err));
    if (r) return hop_set_err(c, r, "%s: access unit %d: %s", who, k, strip_prefix(err, "hop_access_unit_read: "));
  }
  // 3. one parse over the stack; 4. parts, SAO parameters and parser states to the host; 5. the levels only for a caller who asks
  std::vector<hop_cu_part> own_parts; std::vector<hop_sao_param> own_sao;
  if (!parts) { own_parts.resize(n * 256); parts = own_parts.data(); }
  if (sao_on && !sao_coded) { own_sao.resize(n * 3); sao_coded = own_sao.data(); }
  hop_parse_where where = { nullptr, nullptr, 0 };
  std::vector<int32_t> au_qp(n_au);                                       // every access unit's own QP, handed down as an array: the context's table (hop_ctx_set_picture_qps) is neither read nor changed
  for (int k = 0; k < n_au; k++) au_qp[k] = a[k].info.params.slice.qp;
  r = hop_parse_device_at(c, who, "access unit", &sl, nullptr, (const uint8_t*)b, offs.data(), sizes.data(), n_sub, parts, levels, sao_on ? sao_coded : nullptr, front, &where, au_qp.data());
  if (r) return r;
  if (where.end > o_order || (char*)c->scratch != b) return hop_set_err(c, HOP_ERR_STATE, "%s: the parser's work area ends at %zu, %zu were kept for it", who, where.end, o_order);
  // 6. one decode over the parts and levels where the parser left them, one deblocking pass
  hop_dec_params dp; dp.qp = sl.qp; dp.cb_qp_offset = 0; dp.cr_qp_offset = 0; dp.plain_intra = sl.plain_intra; dp.schedule = 0;
  r = hop_dec_device(c, who, "access unit", &dp, parts, nullptr, where.d_parts, where.d_levels, (int32_t*)(b + o_order), au_qp.data()); if (r) return r;
  hop_deblock_params db; db.qp = sl.qp; db.beta_offset_div2 = 0; db.tc_offset_div2 = 0; db.cb_qp_offset = 0; db.cr_qp_offset = 0; db.disable = 0;
  r = hop_dbk_device(c, &db, parts, au_qp.data()); if (r) return r;
  // 7. the SAO parameters resolved per picture (a merge never leaves its picture), one apply
  if (sao_on) {
    std::vector<hop_sao_param> recon(n * 3);
    for (int k = 0; k < n_pic; k++)
      if (hop_sao_reconstruct_params(n_ctu, wctu, c->bd_y, sao_coded + (size_t)k * n_ctu * 3, recon.data() + (size_t)k * n_ctu * 3))
        return hop_set_err(c, HOP_ERR_ARG, "%s: access unit %d: the coded SAO parameters name a merge candidate that is not there", who, k);
    r = hop_sao_apply(c, recon.data()); if (r) return r;
  }
  // 8. the hash of every picture, once per method the SEIs use, against each access unit's own
  for (int k = 0; k < n_au; k++) hash_match[k][0] = hash_match[k][1] = hash_match[k][2] = -1;
  for (int method = 1; method <= 3; method += 2) {
    bool used = false;
    for (int k = 0; k < n_au; k++) used = used || a[k].info.params.hash == method;
    if (!used) continue;
    std::vector<uint8_t> got((size_t)n_pic * 3 * 16);
    r = hop_picture_hash(c, method, (uint8_t (*)[16])got.data()); if (r) return r;
    for (int k = 0; k < n_au; k++)
      if (a[k].info.params.hash == method) for (int comp = 0; comp < 3; comp++) hash_match[k][comp] = !memcmp(&got[((size_t)k * 3 + comp) * 16], a[k].digest[comp], 16);
  }
  for (int k = 0; k < n_au; k++) info[k] = a[k].info;
  return HOP_OK;
}
