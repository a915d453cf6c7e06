// quant_flat_check.cpp -- the host build of the leaf step's plain quantiser (hevc-hop_amd/host/hop_quant_flat_host.cpp over csrc/k_quant_flat_dev.inl) as a stand-alone
// program, meant for the sanitizers:
//   g++ -std=c++14 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/quant_flat_check.cpp \
//       hevc-hop_amd/host/hop_quant_flat_host.cpp hevc-hop_amd/host/hop_hostlogic.cpp -o quant_flat_check && ./quant_flat_check blocks.bin
// blocks.bin is what tools/quant_flat_dump.py writes: the reference's own blocks of tests/golden/quant_flat.npz and quant_flat_sbh.npz and the crafted corners of
// tests/quant_mode_util.py, each with the levels and the sum expected.  Every block goes through hop_quant_flat_tu_host with 1, 16, 64, 256 and 1024 lanes in both lane
// orders, into a buffer of exactly N * N levels.  Exit status 1 if any byte differs (tests/test_quant_mode_cpu.py builds and runs this program).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/hophip.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s blocks.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  static const int lanes[5] = { 1, 16, 64, 256, 1024 };
  int32_t head[2];
  if (fread(head, 4, 2, f) != 2 || head[0] != 0x51464C54 || head[1] < 0) { fprintf(stderr, "not a block file\n"); return 2; }
  int wrong = 0;
  for (int b = 0; b < head[1]; b++) {
    int32_t p[7];                                                       // bit_depth, qp_scaled, i_slice, log2_size, sign_hide, scan_idx, abs_sum
    if (fread(p, 4, 7, f) != 7 || p[3] < 2 || p[3] > 5) { fprintf(stderr, "block %d: short file\n", b); return 2; }
    const size_t n = (size_t)1 << (2 * p[3]);
    std::vector<int32_t> src(n), want(n);
    if (fread(src.data(), 4, n, f) != n || fread(want.data(), 4, n, f) != n) { fprintf(stderr, "block %d: short file\n", b); return 2; }
    for (int li = 0; li < 5; li++)
      for (int desc = 0; desc < 2; desc++) {
        std::vector<int32_t> got(n, 0x55555555); uint32_t sum = 0xAAAAAAAAu;
        if (hop_quant_flat_tu_host(p[0], p[1], p[2], p[3], p[4], p[5], src.data(), got.data(), &sum, lanes[li], desc) || sum != (uint32_t)p[6] || memcmp(got.data(), want.data(), n * 4)) {
          printf("block %d (log2 %d, %d bit, qp %d, scan %d, hide %d): differs with %d lanes, %s\n", b, p[3], p[0], p[1], p[5], p[4], lanes[li], desc ? "descending" : "ascending");
          wrong++;
        }
      }
  }
  fclose(f);
  printf("%d blocks: %d wrong\n", head[1], wrong);
  return wrong ? 1 : 0;
}
