// rdoq_phased_check.cpp -- the host builds of the leaf step's serial stages (hevc-hop_amd/host/hop_rdoq_host.cpp) as a stand-alone program, meant for the sanitizers:
//   g++ -std=c++14 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/rdoq_phased_check.cpp \
//       hevc-hop_amd/host/hop_rdoq_host.cpp hevc-hop_amd/host/hop_hostlogic.cpp -o rdoq_phased_check && ./rdoq_phased_check cases.bin
// cases.bin is what tests/rdoq_cases.py:write_case_file writes (tests/test_rdoq_phased_cpu.py builds and runs this program on the units and context vectors it checks
// through the library).  Every unit goes through rdoq_tu and through the phased form with 1, 64 and 256 lanes in both lane orders, the work areas pre-filled with 0x00 and
// 0xFF; every context vector through both forms of the bit-estimate table.  Exit status 1 if any byte differs.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/hophip.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  static const int lanes[3] = { 1, 64, 256 }, fills[2] = { 0x00, 0xFF };
  int32_t head[2];
  if (fread(head, 4, 2, f) != 2 || head[0] != 0x51445248 || head[1] < 0) { fprintf(stderr, "not a case file\n"); return 2; }
  int wrong = 0;
  const int n_units = head[1];
  for (int u = 0; u < n_units; u++) {
    hop_rdoq_job job; hop_estbits eb;
    if (fread(&job, sizeof(job), 1, f) != 1 || fread(&eb, sizeof(eb), 1, f) != 1 || job.log2_size < 2 || job.log2_size > 5) { fprintf(stderr, "unit %d: short file\n", u); return 2; }
    const size_t n = (size_t)1 << (2 * job.log2_size);
    std::vector<int32_t> src(n), want(n), got(n);
    if (fread(src.data(), 4, n, f) != n) { fprintf(stderr, "unit %d: short file\n", u); return 2; }
    uint32_t wsum = 0, gsum = 0;
    if (hop_rdoq_tu_host(&job, &eb, src.data(), want.data(), &wsum, 0)) { printf("unit %d: refused\n", u); wrong++; continue; }
    if (hop_rdoq_tu_host(&job, &eb, src.data(), got.data(), &gsum, 0xFF) || gsum != wsum || memcmp(got.data(), want.data(), n * 4)) { printf("unit %d: rdoq_tu depends on the fill\n", u); wrong++; }
    for (int fi = 0; fi < 2; fi++)
      for (int li = 0; li < 3; li++)
        for (int desc = 0; desc < 2; desc++) {
          std::fill(got.begin(), got.end(), 0x55555555); gsum = 0xAAAAAAAAu;
          if (hop_rdoq_tu_phased_host(&job, &eb, src.data(), got.data(), &gsum, fills[fi], lanes[li], desc) || gsum != wsum || memcmp(got.data(), want.data(), n * 4)) {
            printf("unit %d (log2 %d comp %d scan %d): phased form differs, fill %02x, %d lanes, %s\n", u, job.log2_size, job.comp, job.scan_idx, fills[fi], lanes[li], desc ? "descending" : "ascending");
            wrong++;
          }
        }
  }
  int32_t n_ctx = 0;
  if (fread(&n_ctx, 4, 1, f) != 1 || n_ctx < 0) { fprintf(stderr, "no context vectors\n"); return 2; }
  for (int v = 0; v < n_ctx; v++) {
    int32_t lc[2]; hop_cabac_ctx ctx;
    if (fread(lc, 4, 2, f) != 2 || fread(ctx.state, 1, sizeof(ctx.state), f) != sizeof(ctx.state)) { fprintf(stderr, "vector %d: short file\n", v); return 2; }
    hop_tu_rd_job job; memset(&job, 0, sizeof(job)); job.log2_size = lc[0]; job.comp = lc[1];
    hop_estbits want, got;
    memset(&want, 0x33, sizeof(want));
    if (hop_estbits_setup_host(&job, &ctx, &want)) { printf("vector %d: refused\n", v); wrong++; continue; }
    for (int fi = 0; fi < 2; fi++)
      for (int li = 0; li < 3; li++)
        for (int desc = 0; desc < 2; desc++) {
          memset(&got, fills[fi], sizeof(got));
          if (hop_estbits_fill_host(&job, &ctx, &got, lanes[li], desc) || memcmp(&got, &want, sizeof(want))) {
            printf("vector %d (log2 %d comp %d): cooperative table differs, fill %02x, %d lanes\n", v, lc[0], lc[1], fills[fi], lanes[li]);
            wrong++;
          }
        }
  }
  fclose(f);
  printf("%d units, %d context vectors: %d wrong\n", n_units, (int)n_ctx, wrong);
  return wrong ? 1 : 0;
}
