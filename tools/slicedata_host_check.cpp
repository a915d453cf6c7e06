// tools/slicedata_host_check.cpp -- the host build of the slice-data writer under the sanitizers: a stand-alone program around hop_slice_data_write_host.
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/slicedata_host_check.cpp hevc-hop_amd/host/hop_entropy.cpp \
//       hevc-hop_amd/host/hop_decode.cpp hevc-hop_amd/host/hop_hostlogic.cpp -o slicedata_host_check
//   ./slicedata_host_check case.dump          (tools/slicedata_dump.py <case> case.dump writes the file from the CPU path of tests/slicedata_cpu.py)
// The dump: 16 int32 -- pic_w, pic_h, bit_depth, the 7 fields of hop_slice_data_params, n_ctu, has_sao, n_substreams, n_bytes, 0, 0 --, then 256 hop_cu_part per CTU,
// 6144 int32 levels per CTU, 3 hop_sao_param per CTU if has_sao, n_substreams uint32 sizes, n_bytes of expected slice data.
// The program writes into a heap buffer of exactly n_bytes (a store past out_capacity is a heap-buffer-overflow report), compares bytes and sizes, then asks for one
// byte less and expects the refusal with the needed size.  Exit status 0: all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hophip.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s case.dump\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t h[16];
  if (!rd(f, h, sizeof(h))) { fprintf(stderr, "short header\n"); return 2; }
  const int w = h[0], ht = h[1], bd = h[2], n_ctu = h[10], has_sao = h[11], n_sub = h[12], n_bytes = h[13];
  hop_slice_data_params p; memcpy(&p, h + 3, sizeof(p));
  if (n_ctu != ((w + 63) / 64) * ((ht + 63) / 64) || n_sub < 1 || n_bytes < 1) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<hop_cu_part> parts((size_t)n_ctu * 256);
  std::vector<int32_t> levels((size_t)n_ctu * 6144);
  std::vector<hop_sao_param> sao(has_sao ? (size_t)n_ctu * 3 : 0);
  std::vector<uint32_t> want_sizes(n_sub);
  std::vector<uint8_t> want(n_bytes);
  if (!rd(f, parts.data(), parts.size() * sizeof(hop_cu_part)) || !rd(f, levels.data(), levels.size() * 4) || !rd(f, sao.data(), sao.size() * sizeof(hop_sao_param)) ||
      !rd(f, want_sizes.data(), want_sizes.size() * 4) || !rd(f, want.data(), want.size())) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);
  const int rows = (ht + 63) / 64;
  for (int pass = 0; pass < 2; pass++) {
    const size_t cap = (size_t)n_bytes - pass;                          // exactly enough, then one byte short
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    std::vector<uint32_t> sizes(rows, 0);
    int32_t ns = -1;
    const int rc = hop_slice_data_write_host(w, ht, bd, &p, parts.data(), levels.data(), has_sao ? sao.data() : NULL, out, cap, sizes.data(), &ns);
    bool ok;
    if (pass == 0) ok = rc == HOP_OK && ns == n_sub && !memcmp(out, want.data(), n_bytes) && !memcmp(sizes.data(), want_sizes.data(), 4 * (size_t)n_sub);
    else ok = rc == HOP_ERR_ARG && ns == n_bytes;
    free(out);
    if (!ok) { fprintf(stderr, "%s: pass %d: status %d, n_substreams %d\n", argv[1], pass, rc, ns); return 1; }
  }
  printf("%s: %d bytes in %d substreams as expected; one byte less refused\n", argv[1], n_bytes, n_sub);
  return 0;
}
