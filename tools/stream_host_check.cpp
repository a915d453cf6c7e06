// tools/stream_host_check.cpp -- the host code of the stream's outer layer under the sanitizers: a stand-alone program around hop_access_unit_write_host,
// hop_parameter_sets_write and hop_rbsp_escape_host.
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/stream_host_check.cpp hevc-hop_amd/host/hop_stream.cpp \
//       hevc-hop_amd/host/hop_entropy.cpp hevc-hop_amd/host/hop_decode.cpp hevc-hop_amd/host/hop_hostlogic.cpp -o stream_host_check
//   ./stream_host_check case.dump ...          (tools/stream_dump.py <case> <picture> case.dump: a picture coded on the CPU and the reference encoder's access unit)
//   ./stream_host_check --escape escape.dump   (tools/stream_dump.py --escape escape.dump: the crafted escape inputs with the restatement's results)
// Every output goes into a heap buffer of exactly the expected size (a store past the capacity is a heap-buffer-overflow report), is compared, and is asked for again
// with one byte less, which must be refused with the size needed.  Exit status 0: all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hophip.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int check_escape(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return 2; }
  int n_rec = 0;
  for (;;) {
    uint32_t h[3];
    if (!rd(f, h, sizeof(h))) { fprintf(stderr, "short file\n"); return 2; }
    if (!h[0]) break;
    const uint32_t n = h[0], n_seg = h[1], want_len = h[2];
    std::vector<uint32_t> seg(n_seg), want_cnt(n_seg), cnt(n_seg);
    std::vector<uint8_t> data(n), want(want_len);
    if (!rd(f, seg.data(), 4 * (size_t)n_seg) || !rd(f, want_cnt.data(), 4 * (size_t)n_seg) || !rd(f, data.data(), n) || !rd(f, want.data(), want_len)) { fprintf(stderr, "short record\n"); return 2; }
    for (int pass = 0; pass < 2; pass++) {
      const size_t cap = want_len - pass;
      uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
      size_t got = 0;
      const int rc = hop_rbsp_escape_host(data.data(), seg.data(), (int32_t)n_seg, out, cap, &got, cnt.data());
      const bool ok = pass == 0 ? rc == HOP_OK && got == want_len && !memcmp(out, want.data(), want_len) && !memcmp(cnt.data(), want_cnt.data(), 4 * (size_t)n_seg)
                                : rc == HOP_ERR_ARG && got == want_len && !memcmp(out, want.data(), cap);
      free(out);
      if (!ok) { fprintf(stderr, "%s: record %d (%u bytes, %u segments) pass %d: status %d, %zu bytes\n", path, n_rec, n, n_seg, pass, rc, got); return 1; }
    }
    n_rec++;
  }
  fclose(f);
  printf("%s: %d escape records as expected; one byte less refused\n", path, n_rec);
  return 0;
}

static int check_picture(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return 2; }
  int32_t h[16];
  if (!rd(f, h, sizeof(h))) { fprintf(stderr, "short header\n"); return 2; }
  const int w = h[0], ht = h[1], bd = h[2], n_ctu = h[13], has_sao = h[14], n_bytes = h[15];
  hop_stream_params p; memcpy(&p, h + 3, sizeof(p));
  if (n_ctu != ((w + 63) / 64) * ((ht + 63) / 64) || n_bytes < 1 || sizeof(p) != 40) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<hop_cu_part> parts((size_t)n_ctu * 256);
  std::vector<int32_t> levels((size_t)n_ctu * 6144);
  std::vector<hop_sao_param> sao(has_sao ? (size_t)n_ctu * 3 : 0);
  std::vector<int16_t> y((size_t)w * ht), cb((size_t)w * ht / 4), cr((size_t)w * ht / 4);
  std::vector<uint8_t> want(n_bytes);
  if (!rd(f, parts.data(), parts.size() * sizeof(hop_cu_part)) || !rd(f, levels.data(), levels.size() * 4) || !rd(f, sao.data(), sao.size() * sizeof(hop_sao_param)) ||
      !rd(f, y.data(), y.size() * 2) || !rd(f, cb.data(), cb.size() * 2) || !rd(f, cr.data(), cr.size() * 2) || !rd(f, want.data(), want.size())) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);
  const int16_t* rec[3] = { y.data(), cb.data(), cr.data() };
  for (int pass = 0; pass < 2; pass++) {
    const size_t cap = (size_t)n_bytes - pass;                          // exactly enough, then one byte short
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    size_t got = 0;
    const int rc = hop_access_unit_write_host(w, ht, bd, &p, parts.data(), levels.data(), has_sao ? sao.data() : NULL, p.hash ? rec : NULL, out, cap, &got);
    const bool ok = pass == 0 ? rc == HOP_OK && got == (size_t)n_bytes && !memcmp(out, want.data(), n_bytes) : rc == HOP_ERR_ARG && got == (size_t)n_bytes;
    free(out);
    if (!ok) { fprintf(stderr, "%s: pass %d: status %d, %zu bytes (expected %d)\n", path, pass, rc, got, n_bytes); return 1; }
  }
  if (p.parameter_sets) {                                               // the parameter sets alone: the head of the access unit
    for (int pass = 0; pass < 2; pass++) {
      size_t got = 0, cap = 256;
      std::vector<uint8_t> probe(cap);
      if (hop_parameter_sets_write(w, ht, bd, &p, probe.data(), cap, &got) != HOP_OK || got > (size_t)n_bytes) { fprintf(stderr, "%s: parameter sets\n", path); return 1; }
      cap = got - pass;
      uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
      size_t again = 0;
      const int rc = hop_parameter_sets_write(w, ht, bd, &p, out, cap, &again);
      const bool ok = pass == 0 ? rc == HOP_OK && again == got && !memcmp(out, want.data(), got) : rc == HOP_ERR_ARG && again == got;
      free(out);
      if (!ok) { fprintf(stderr, "%s: parameter sets pass %d: status %d, %zu bytes\n", path, pass, rc, again); return 1; }
    }
  }
  printf("%s: access unit of %d bytes as expected; one byte less refused\n", path, n_bytes);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s case.dump ... | --escape escape.dump\n", argv[0]); return 2; }
  if (!strcmp(argv[1], "--escape")) return argc == 3 ? check_escape(argv[2]) : 2;
  for (int i = 1; i < argc; i++) { const int r = check_picture(argv[i]); if (r) return r; }
  return 0;
}
