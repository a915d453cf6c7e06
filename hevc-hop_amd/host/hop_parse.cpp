// hop_parse.cpp -- host side of the slice-data parser (plain C++, no device code): the checks hop_slice_data_parse runs before anything is enqueued, and
// hop_slice_data_parse_host -- the body of csrc/k_parse_dev.inl compiled for the host.  Like hop_slice_data_write_host the host entry is a yardstick, what the CPU tests
// and the sanitizer program (tools/slicedata_parse_check.cpp) drive; it is not a CPU path of the product: hop_slice_data_parse always launches kernels (csrc/k_parse.hip).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/hophip.h"

#define ENT_FN static inline
#define ENT_TAB static const
#include "../csrc/k_entropy_dev.inl"
#include "../csrc/k_parse_dev.inl"

void hop_rdoq_build_scans(uint16_t* tabs /* 4080 + 255 entries */);   // host/hop_hostlogic.cpp
extern "C" {
int hop_ent_init_states(uint8_t st[EN_STATES], int slice_type, int qp);   // host/hop_entropy.cpp

// internal: everything both entries refuse before they start -- the parameters (the writer's, and a micro-image size the candidates can be derived with), the number of
// substreams, their sizes.  *total = the bytes of all n_pic * n_substreams substreams
__attribute__((visibility("hidden"))) int hop_parse_check(int pic_w, int pic_h, int bit_depth, int n_pic, const hop_slice_data_params* p, const uint8_t* data,
                                                          const uint32_t* substream_bytes, int n_substreams, const hop_cu_part* parts, const hop_sao_param* sao,
                                                          size_t* total, char* err, size_t errn) {
#define REFUSE(...) do { if (err && errn) snprintf(err, errn, "hop_slice_data_parse: " __VA_ARGS__); return HOP_ERR_ARG; } while (0)
  if (err && errn) err[0] = 0;
  if (pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7) || pic_w > 65536 || pic_h > 65536 || bit_depth < 8 || bit_depth > 12 || n_pic < 1 || n_pic > 65536 || !p || !data ||
      !substream_bytes || !parts || !total)
    REFUSE("bad argument");
  if (p->slice_type < 0 || p->slice_type > 4 || p->qp < -6 * (bit_depth - 8) || p->qp > 51 || (p->wpp != 0 && p->wpp != 1) || (p->plain_intra != 0 && p->plain_intra != 1) ||
      (p->sao_luma != 0 && p->sao_luma != 1) || (p->sao_chroma != 0 && p->sao_chroma != 1) || p->mi_size < 0)
    REFUSE("parameter out of range");
  if ((p->plain_intra != 0) != (p->slice_type == 2)) REFUSE("plain_intra goes with slice type I (2), the HOP configuration with the others");
  if (!p->plain_intra && bit_depth != 8) REFUSE("the HOP configuration is 8 bit");
  if (!p->plain_intra && (p->mi_size < 1 || p->mi_size > 4096)) REFUSE("mi_size %d: the micro-image candidates need 1..4096", p->mi_size);
  if (((p->sao_luma || p->sao_chroma) != 0) != (sao != NULL)) REFUSE("sao_coded and the SAO flags disagree");
  const int hctu = (pic_h + 63) / 64;
  if (n_substreams != (p->wpp ? hctu : 1)) REFUSE("n_substreams is %d, the picture has %d", n_substreams, p->wpp ? hctu : 1);
  size_t sum = 0;
  for (size_t i = 0; i < (size_t)n_pic * n_substreams; i++) {
    if (substream_bytes[i] == 0) REFUSE("substream %zu is empty", i);
    if (sum + substream_bytes[i] < sum) REFUSE("the substream sizes overflow");
    sum += substream_bytes[i];
  }
  *total = sum;
  return HOP_OK;
#undef REFUSE
}

int hop_slice_data_parse_host(int pic_w, int pic_h, int bit_depth, const hop_slice_data_params* p, const uint8_t* data, const uint32_t* substream_bytes,
                              int32_t n_substreams, hop_cu_part* parts, int32_t* levels, hop_sao_param* sao) {
  size_t total = 0;
  const int rc = hop_parse_check(pic_w, pic_h, bit_depth, 1, p, data, substream_bytes, n_substreams, parts, sao, &total, NULL, 0);
  if (rc) return rc;
  std::vector<uint16_t> scans(4080 + 255);
  hop_rdoq_build_scans(scans.data());
  ParPic g;
  g.e.pic_w = pic_w; g.e.pic_h = pic_h; g.e.wctu = (pic_w + 63) / 64; g.e.hctu = (pic_h + 63) / 64;
  g.e.i_slice = p->slice_type == 2; g.e.sao_luma = p->sao_luma; g.e.sao_chroma = p->sao_chroma; g.e.sao_max_offset = (1 << ((bit_depth < 10 ? bit_depth : 10) - 5)) - 1;
  g.e.parts = parts; g.e.levels = levels; g.e.sao = sao; g.e.scans = scans.data();
  g.wpp = p->wpp; g.sao_shift = bit_depth - (bit_depth < 10 ? bit_depth : 10); g.mi_size = p->mi_size; g.mi_merge = !p->plain_intra;
  g.parts = parts; g.levels = levels; g.sao = sao;
  const int n = g.e.wctu * g.e.hctu;
  for (size_t i = 0; i < (size_t)n * 256; i++) pa_unit_init(parts[i], 0);
  if (levels) memset(levels, 0, sizeof(int32_t) * 6144 * (size_t)n);
  if (sao) memset(sao, 0, sizeof(hop_sao_param) * 3 * (size_t)n);
  uint8_t init[EN_STATES];
  if (hop_ent_init_states(init, p->slice_type, p->qp)) return HOP_ERR_ARG;
  // the rows in order: row r + 1 starts from the models row r holds after its second CTU -- from the initial ones in a picture one CTU wide (TDecSlice.cpp:237-264, :371)
  std::vector<uint8_t> entry(init, init + EN_STATES);
  ParDec k; memset(&k, 0, sizeof(k));
  int bad = 0;
  size_t at = 0;
  for (int s = 0; s < n_substreams; s++) {
    pa_begin_substream(k, entry.data(), data + at, substream_bytes[s]);
    const int first = p->wpp ? s * g.e.wctu : 0, count = p->wpp ? g.e.wctu : n;
    if (p->wpp && g.e.wctu < 2) entry.assign(init, init + EN_STATES);
    for (int a = first; a < first + count; a++) {
      pa_parse_ctu(k, g, a);
      if (p->wpp && a == first + 1) entry.assign(k.st, k.st + EN_STATES);
    }
    if (k.flags) bad = 1;
    at += substream_bytes[s];
  }
  return bad ? HOP_ERR_ARG : HOP_OK;
}

}  // extern "C"
