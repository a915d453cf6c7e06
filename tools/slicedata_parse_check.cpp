// tools/slicedata_parse_check.cpp -- the host build of the slice-data parser under the sanitizers: a stand-alone program around hop_slice_data_parse_host.
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/slicedata_parse_check.cpp hevc-hop_amd/host/hop_parse.cpp \
//       hevc-hop_amd/host/hop_entropy.cpp hevc-hop_amd/host/hop_decode.cpp hevc-hop_amd/host/hop_hostlogic.cpp -o slicedata_parse_check
//   ./slicedata_parse_check case.dump          (tools/slicedata_dump.py <case> case.dump writes the file; the layout is described in tools/slicedata_host_check.cpp)
// (a) the dump's bytes -- the reference encoder's slice data -- are parsed from a heap copy of exactly n_bytes into heap outputs of exactly their sizes (a load or store
//     past either is a heap-buffer-overflow report) and compared with the dump's parts, levels and SAO parameters; one field is not compared on some units: gt_flag on the
//     units of an SS / GT CU that are not a PU's first unit (include/hophip.h says why);
// (b) the parsed result goes back through hop_slice_data_write_host and must give the bytes and sizes;
// (c) 100 damaged streams -- the generator of tests/slicedata_parse_util.py (variants, case_seed), restated -- must each end in HOP_OK or HOP_ERR_ARG; what came back as
//     HOP_OK goes through hop_decode_schedule, which accepts or refuses it.
// Exit status 0: all as expected.  Host code only: run it on the CPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hophip.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int zidx(int x4, int y4) { int z = 0; for (int b = 0; b < 4; b++) z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1)); return z; }
static void zpos(int z, int& x4, int& y4) { x4 = y4 = 0; for (int b = 0; b < 4; b++) { x4 |= ((z >> (2 * b)) & 1) << b; y4 |= ((z >> (2 * b + 1)) & 1) << b; } }

// the units of a CTU that are the first unit of a PU of an SS / GT CU
static void pu_first_units(const hop_cu_part* ctu, bool first[256]) {
  memset(first, 0, 256);
  for (int z = 0; z < 256;) {
    const hop_cu_part& u = ctu[z];
    if (u.pred_mode == 15) { z++; continue; }
    if (u.pred_mode == 0) {
      first[z] = true;
      const int s4 = (64 >> u.depth) >> 2;
      int ox = -1, oy = 0;
      switch (u.part_size) {
        case 1: ox = 0; oy = s4 >> 1; break;  case 2: ox = s4 >> 1; break;
        case 4: ox = 0; oy = s4 >> 2; break;  case 5: ox = 0; oy = (s4 >> 2) + (s4 >> 1); break;
        case 6: ox = s4 >> 2; break;          case 7: ox = (s4 >> 2) + (s4 >> 1); break;
        default: break;
      }
      if (ox >= 0) { int x4, y4; zpos(z, x4, y4); first[zidx(x4 + ox, y4 + oy)] = true; }
    }
    z += 256 >> (2 * u.depth);
  }
}

struct Lcg { unsigned long long s; unsigned long long next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; } };

struct Outputs {
  hop_cu_part* parts; int32_t* levels; hop_sao_param* sao;
  Outputs(int n_ctu, bool has_sao) {
    parts = (hop_cu_part*)malloc(sizeof(hop_cu_part) * 256 * (size_t)n_ctu); levels = (int32_t*)malloc(sizeof(int32_t) * 6144 * (size_t)n_ctu);
    sao = has_sao ? (hop_sao_param*)malloc(sizeof(hop_sao_param) * 3 * (size_t)n_ctu) : NULL;
  }
  ~Outputs() { free(parts); free(levels); free(sao); }
};

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
  std::vector<uint32_t> sizes(n_sub);
  std::vector<uint8_t> bytes(n_bytes);
  if (!rd(f, parts.data(), parts.size() * sizeof(hop_cu_part)) || !rd(f, levels.data(), levels.size() * 4) || !rd(f, sao.data(), sao.size() * sizeof(hop_sao_param)) ||
      !rd(f, sizes.data(), sizes.size() * 4) || !rd(f, bytes.data(), bytes.size())) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);
  {                                                                       // (a), (b)
    uint8_t* in = (uint8_t*)malloc(n_bytes); memcpy(in, bytes.data(), n_bytes);
    Outputs o(n_ctu, has_sao != 0);
    const int rc = hop_slice_data_parse_host(w, ht, bd, &p, in, sizes.data(), n_sub, o.parts, o.levels, o.sao);
    free(in);
    if (rc != HOP_OK) { fprintf(stderr, "%s: parse: status %d\n", argv[1], rc); return 1; }
    if (memcmp(o.levels, levels.data(), levels.size() * 4)) { fprintf(stderr, "%s: levels differ\n", argv[1]); return 1; }
    if (has_sao && memcmp(o.sao, sao.data(), sao.size() * sizeof(hop_sao_param))) { fprintf(stderr, "%s: SAO parameters differ\n", argv[1]); return 1; }
    for (int a = 0; a < n_ctu; a++) {
      bool first[256]; pu_first_units(&parts[(size_t)a * 256], first);
      for (int z = 0; z < 256; z++) {
        hop_cu_part got = o.parts[(size_t)a * 256 + z]; const hop_cu_part& want = parts[(size_t)a * 256 + z];
        if (want.pred_mode == 0 && !first[z]) got.gt_flag = want.gt_flag;
        if (memcmp(&got, &want, sizeof(got))) { fprintf(stderr, "%s: CTU %d unit %d differs\n", argv[1], a, z); return 1; }
      }
    }
    uint8_t* out = (uint8_t*)malloc(n_bytes);
    std::vector<uint32_t> back((ht + 63) / 64, 0); int32_t ns = -1;
    const int wc = hop_slice_data_write_host(w, ht, bd, &p, o.parts, o.levels, o.sao, out, n_bytes, back.data(), &ns);
    const bool same = wc == HOP_OK && ns == n_sub && !memcmp(out, bytes.data(), n_bytes) && !memcmp(back.data(), sizes.data(), 4 * (size_t)n_sub);
    free(out);
    if (!same) { fprintf(stderr, "%s: write after parse: status %d, n_substreams %d\n", argv[1], wc, ns); return 1; }
  }
  int n_ok = 0, n_err = 0, n_sched = 0;
  Lcg g; g.s = (unsigned long long)w * 65536 + ht;                        // (c)
  for (int i = 0; i < 100; i++) {
    const unsigned long long r1 = g.next(), r2 = g.next();
    uint8_t* in = (uint8_t*)malloc(n_bytes); memcpy(in, bytes.data(), n_bytes);
    std::vector<uint32_t> s(sizes);
    int kind = i % 5;
    if (kind == 4 && n_sub < 2) kind = 1;
    const size_t at = (size_t)(r1 % (unsigned long long)n_bytes);
    if (kind == 0) in[at] = (uint8_t)(r2 & 255);
    else if (kind == 1) in[at] ^= (uint8_t)(1u << (r2 % 8));
    else if (kind == 2) memset(in + at, 0, n_bytes - at);
    else if (kind == 3) memset(in + at, 0xFF, n_bytes - at);
    else { const int a = (int)(r1 % n_sub), b = (int)((a + 1 + r2 % (n_sub - 1)) % n_sub); const uint32_t t = s[a]; s[a] = s[b]; s[b] = t; }
    Outputs o(n_ctu, has_sao != 0);
    const int rc = hop_slice_data_parse_host(w, ht, bd, &p, in, s.data(), n_sub, o.parts, o.levels, o.sao);
    free(in);
    if (rc != HOP_OK && rc != HOP_ERR_ARG) { fprintf(stderr, "%s: variant %d (kind %d): status %d\n", argv[1], i, kind, rc); return 1; }
    if (rc == HOP_OK) {
      n_ok++;
      std::vector<int32_t> lv(n_ctu); int32_t nl = 0;
      const int sc = hop_decode_schedule(w, ht, o.parts, 0, lv.data(), &nl);
      if (sc != HOP_OK && sc != HOP_ERR_ARG) { fprintf(stderr, "%s: variant %d (kind %d): hop_decode_schedule %d\n", argv[1], i, kind, sc); return 1; }
      n_sched += sc == HOP_OK;
    } else n_err++;
  }
  printf("%s: %d bytes in %d substreams parsed as expected and written back; 100 damaged streams: %d HOP_OK (%d accepted by hop_decode_schedule), %d HOP_ERR_ARG\n",
         argv[1], n_bytes, n_sub, n_ok, n_sched, n_err);
  return 0;
}
