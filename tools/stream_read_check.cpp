// tools/stream_read_check.cpp -- the host code of the stream reader under the sanitizers: a stand-alone program around hop_access_unit_read_host, hop_annexb_access_unit
// and hop_rbsp_unescape_host.
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/stream_read_check.cpp hevc-hop_amd/host/hop_stream_read.cpp \
//       -o stream_read_check
//   ./stream_read_check read.dump          (tools/stream_read_dump.py read.dump: the fixture streams' access units, the crafted ones, the unescape inputs)
// Every input is copied into a heap buffer of exactly its size (a read past au_bytes is a heap-buffer-overflow report) and every output goes into one of exactly the
// size it takes (so is a store past a capacity).  Per access unit: the read must succeed and repeat into exact buffers; one byte less of data and one substream less are
// refused with the size needed; then every prefix and 100 seeded single-byte changes (the generator of tests/stream_read_util.damage) must each be read or refused.
// Per unescape record: output, per-segment sizes and violations as the dump expects; one byte less refused.  Exit status 0: all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hophip.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool same(const void* a, const void* b, size_t n) { return n == 0 || !memcmp(a, b, n); }

// one read with the access unit and every output in exact-size heap blocks; returns the status, *need the slice data's size
static int read_exact(const uint8_t* au, size_t n, const hop_stream_info* active, size_t cap, int max_sub, size_t* need, hop_stream_info* info_out, std::vector<uint8_t>* data_out,
                      std::vector<uint32_t>* sizes_out) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1); memcpy(in, au, n);
  uint8_t* data = (uint8_t*)malloc(cap ? cap : 1);
  uint32_t* sizes = (uint32_t*)malloc(sizeof(uint32_t) * (max_sub > 0 ? max_sub : 1));
  uint8_t (*digest)[16] = (uint8_t (*)[16])malloc(48);
  hop_stream_info* info = (hop_stream_info*)malloc(sizeof(hop_stream_info));
  size_t got = 0;
  const int rc = hop_access_unit_read_host(in, n, active, info, data, cap, &got, sizes, max_sub, digest);
  if (need) *need = got;
  if (rc == HOP_OK) {
    if (info_out) *info_out = *info;
    if (data_out) data_out->assign(data, data + got);
    if (sizes_out) sizes_out->assign(sizes, sizes + info->n_substreams);
  }
  free(in); free(data); free(sizes); free(digest); free(info);
  return rc;
}

static int check_unit(int rec, const std::vector<uint8_t>& au, const hop_stream_info* active, uint32_t seed, bool prefixes, long* n_calls) {
  size_t need = 0; hop_stream_info info; std::vector<uint8_t> data, again; std::vector<uint32_t> sizes, sizes2;
  if (read_exact(au.data(), au.size(), active, au.size(), 4096, &need, &info, &data, &sizes) != HOP_OK) { fprintf(stderr, "record %d: not read\n", rec); return 1; }
  size_t sum = 0; for (size_t i = 0; i < sizes.size(); i++) sum += sizes[i];
  if (sum != need || data.size() != need || info.n_substreams != (int32_t)sizes.size()) { fprintf(stderr, "record %d: sizes do not add up\n", rec); return 1; }
  if (read_exact(au.data(), au.size(), active, need, info.n_substreams, NULL, NULL, &again, &sizes2) != HOP_OK || again != data || sizes2 != sizes) { fprintf(stderr, "record %d: exact buffers\n", rec); return 1; }
  size_t n2 = 0;
  if (read_exact(au.data(), au.size(), active, need - 1, info.n_substreams, &n2, NULL, NULL, NULL) != HOP_ERR_ARG || n2 != need) { fprintf(stderr, "record %d: one byte less not refused with the size\n", rec); return 1; }
  if (read_exact(au.data(), au.size(), active, need, info.n_substreams - 1, NULL, NULL, NULL, NULL) != HOP_ERR_ARG) { fprintf(stderr, "record %d: one substream less not refused\n", rec); return 1; }
  size_t first = 0;
  { uint8_t* in = (uint8_t*)malloc(au.size()); memcpy(in, au.data(), au.size());
    const int rc = hop_annexb_access_unit(in, au.size(), &first); free(in);
    if (rc != HOP_OK || first != au.size()) { fprintf(stderr, "record %d: hop_annexb_access_unit %d, %zu of %zu\n", rec, rc, first, au.size()); return 1; } }
  *n_calls += 4;
  if (prefixes) for (size_t n = 0; n < au.size(); n++) {
    const int rc = read_exact(au.data(), n, active, n, 4096, NULL, NULL, NULL, NULL);
    if (rc != HOP_OK && rc != HOP_ERR_ARG) { fprintf(stderr, "record %d: prefix %zu: status %d\n", rec, n, rc); return 1; }
    ++*n_calls;
  }
  uint32_t x = seed;
  std::vector<uint8_t> bad(au);
  for (int k = 0; k < 100; k++) {
    x = 1664525u * x + 1013904223u;
    const size_t pos = (x >> 8) % au.size();
    x = 1664525u * x + 1013904223u;
    uint8_t v = (uint8_t)(x >> 16);
    if (v == au[pos]) v ^= 1;
    bad[pos] = v;
    const int rc = read_exact(bad.data(), bad.size(), active, bad.size(), 4096, NULL, NULL, NULL, NULL);
    bad[pos] = au[pos];
    if (rc != HOP_OK && rc != HOP_ERR_ARG) { fprintf(stderr, "record %d: change %d at %zu: status %d\n", rec, k, pos, rc); return 1; }
    ++*n_calls;
  }
  return 0;
}

static int check_unescape(int rec, FILE* f, const uint32_t h[8]) {
  const uint32_t n = h[1], n_seg = h[2], back = h[3], want_len = h[4], want_viol = h[5];
  std::vector<uint32_t> seg(n_seg), want_sizes(n_seg);
  std::vector<uint8_t> data(n), want(want_len);
  if (!rd(f, seg.data(), 4 * (size_t)n_seg) || !rd(f, want_sizes.data(), 4 * (size_t)n_seg) || !rd(f, data.data(), n) || !rd(f, want.data(), want_len)) { fprintf(stderr, "short record\n"); return 2; }
  for (int pass = 0; pass < 2; pass++) {
    if (pass && !want_len) break;
    const size_t cap = want_len - pass;
    uint8_t* in = (uint8_t*)malloc(n ? n : 1); memcpy(in, data.data(), n);
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    uint32_t* sizes = (uint32_t*)malloc(4 * (size_t)n_seg);
    size_t got = 0; uint32_t viol = 0;
    const int rc = hop_rbsp_unescape_host(in, seg.data(), (int32_t)n_seg, (int32_t)back, out, cap, &got, sizes, &viol);
    const bool ok = pass == 0 ? rc == HOP_OK && got == want_len && same(out, want.data(), want_len) && same(sizes, want_sizes.data(), 4 * (size_t)n_seg) && viol == want_viol
                              : rc == HOP_ERR_ARG && got == want_len && same(out, want.data(), cap);
    free(in); free(out); free(sizes);
    if (!ok) { fprintf(stderr, "record %d (%u bytes, %u segments, lookback %u) pass %d: status %d, %zu bytes\n", rec, n, n_seg, back, pass, rc, got); return 1; }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s read.dump\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int n_units = 0, n_une = 0; long n_calls = 0;
  for (int rec = 0;; rec++) {
    uint32_t h[8];                                              // kind; unit: bytes, seed, has_active, prefixes; unescape: n, n_seg, lookback, want_len, want_viol
    if (!rd(f, h, sizeof(h))) { fprintf(stderr, "short file\n"); return 2; }
    if (h[0] == 0) break;
    if (h[0] == 1) {
      hop_stream_info active;
      std::vector<uint8_t> au(h[1]);
      if ((h[3] && !rd(f, &active, sizeof(active))) || !rd(f, au.data(), au.size()) || au.empty()) { fprintf(stderr, "short record\n"); return 2; }
      const int r = check_unit(rec, au, h[3] ? &active : NULL, h[2], h[4] != 0, &n_calls);
      if (r) return r;
      n_units++;
    } else if (h[0] == 2) {
      const int r = check_unescape(rec, f, h);
      if (r) return r;
      n_une++;
    } else { fprintf(stderr, "record %d: kind %u\n", rec, h[0]); return 2; }
  }
  fclose(f);
  printf("%s: %d access units read into exact buffers, %ld prefixes and single-byte changes read or refused; %d unescape records as expected\n", argv[1], n_units, n_calls, n_une);
  return 0;
}
