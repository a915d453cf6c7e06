// hop_entropy.cpp -- host side of the slice-data writer (plain C++, no device code): the checks hop_slice_data_write runs before anything is enqueued, the initial
// context models, and hop_slice_data_write_host -- the body of csrc/k_entropy_dev.inl compiled for the host.  Like hop_decode_schedule and hop_sao_decide the host entry is
// a yardstick, what the CPU tests drive; it is not a CPU path of the product: hop_slice_data_write always launches kernels (csrc/k_entropy.hip).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/hophip.h"

#define ENT_FN static inline
#define ENT_TAB static const
#include "../csrc/k_entropy_dev.inl"

void hop_rdoq_build_scans(uint16_t* tabs /* 4080 + 255 entries */);   // host/hop_hostlogic.cpp: the tables the device entry keeps in c->rdoq_scans
uint8_t hop_ctx_init_state(int qp, int init_value);                // host/hop_hostlogic.cpp: ContextModel::init
extern "C" {
int hop_dec_plan(int pic_w, int pic_h, int allow_inter, const hop_cu_part* parts, int schedule, int32_t* ctu_level, int32_t* n_levels, char* err, size_t errn);   // host/hop_decode.cpp
}

namespace {
int fail(char* err, size_t n, const char* what, int pic, int ctu, int unit) {
  if (err && n) snprintf(err, n, "hop_slice_data_write: picture %d CTU %d unit %d: %s", pic, ctu, unit, what);
  return HOP_ERR_ARG;
}
}  // namespace

extern "C" {

// internal: the context models a substream starts from -- TEncSbac::resetEntropy (TEncSbac.cpp:136-148) through hop_cabac_init / hop_cabac_cu_init / hop_cabac_split_init,
// and the two SAO models (INIT_SAO_MERGE_FLAG / INIT_SAO_TYPE_IDX, ContextTables.h:488-519; rows B, P, I, ISS, PSS)
__attribute__((visibility("hidden"))) int hop_ent_init_states(uint8_t st[EN_STATES], int slice_type, int qp) {
  static const uint8_t init_merge[5] = { 153, 153, 153, 153, 153 }, init_type[5] = { 160, 185, 200, 185, 185 };
  hop_cabac_ctx r; hop_cabac_cu_ctx cu; uint8_t split[3];
  if (hop_cabac_init(&r, slice_type, qp) || hop_cabac_cu_init(&cu, slice_type, qp) || hop_cabac_split_init(split, slice_type, qp)) return HOP_ERR_ARG;
  memset(st, 0, EN_STATES);
  memcpy(st, r.state, 150); memcpy(st + EN_CU, cu.state, 19); memcpy(st + EN_SPLIT, split, 3);
  st[EN_SAO_MERGE] = hop_ctx_init_state(qp, init_merge[slice_type]); st[EN_SAO_TYPE] = hop_ctx_init_state(qp, init_type[slice_type]);
  return HOP_OK;
}

// internal: everything both entries refuse before they start -- the parameters, the partition data of n_pic pictures (the validators of hop_decode_frame, and what only
// the syntax cares about: merge and predictor indices, skipped CUs, the chroma direction among the allowed ones), host levels beyond 16 bits, the SAO parameters
__attribute__((visibility("hidden"))) int hop_ent_check(int pic_w, int pic_h, int bit_depth, int n_pic, const hop_slice_data_params* p, const hop_cu_part* parts,
                                                        const int32_t* levels, const hop_sao_param* sao, char* err, size_t errn) {
  if (err && errn) err[0] = 0;
  if (pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7) || bit_depth < 8 || bit_depth > 12 || n_pic < 1 || !p || !parts) { if (err && errn) snprintf(err, errn, "hop_slice_data_write: bad argument"); return HOP_ERR_ARG; }
  if (p->slice_type < 0 || p->slice_type > 4 || p->qp < -6 * (bit_depth - 8) || p->qp > 51 || (p->wpp != 0 && p->wpp != 1) || (p->plain_intra != 0 && p->plain_intra != 1) ||
      (p->sao_luma != 0 && p->sao_luma != 1) || (p->sao_chroma != 0 && p->sao_chroma != 1) || p->mi_size < 0) {
    if (err && errn) snprintf(err, errn, "hop_slice_data_write: parameter out of range");
    return HOP_ERR_ARG;
  }
  if ((p->plain_intra != 0) != (p->slice_type == 2)) { if (err && errn) snprintf(err, errn, "hop_slice_data_write: plain_intra goes with slice type I (2), the HOP configuration with the others"); return HOP_ERR_ARG; }
  if (!p->plain_intra && bit_depth != 8) { if (err && errn) snprintf(err, errn, "hop_slice_data_write: the HOP configuration is 8 bit"); return HOP_ERR_ARG; }
  if (((p->sao_luma || p->sao_chroma) != 0) != (sao != NULL)) { if (err && errn) snprintf(err, errn, "hop_slice_data_write: sao_coded and the SAO flags disagree"); return HOP_ERR_ARG; }
  const int wctu = (pic_w + 63) / 64, hctu = (pic_h + 63) / 64, n = wctu * hctu;
  std::vector<int32_t> level(n); int32_t n_levels = 0;
  for (int k = 0; k < n_pic; k++) {
    const hop_cu_part* P = parts + (size_t)k * n * 256;
    const int r = hop_dec_plan(pic_w, pic_h, !p->plain_intra, P, 1, level.data(), &n_levels, err, errn);
    if (r) return r;
    for (int a = 0; a < n; a++) {
      int z = 0;
      while (z < 256) {
        const hop_cu_part& u = P[(size_t)a * 256 + z];
        if (u.pred_mode == 15) { z++; continue; }
        const int np = 256 >> (2 * u.depth);
        {                                                                 // a transform below the CU's smallest (getQuadtreeTULog2MinSizeInCU) has no syntax: the subdivision flag is inferred 0 there
          const int log2_cu = 6 - u.depth, nxn = u.pred_mode == 1 && u.part_size == 3;
          const int log2_min = log2_cu < 4 + nxn ? 2 : (log2_cu - 2 - nxn > 5 ? 5 : log2_cu - 2 - nxn);
          for (int q = 0; q < np; q++) if (log2_cu - P[(size_t)a * 256 + z + q].tr_idx < log2_min) return fail(err, errn, "a transform depth the CU's syntax cannot express", k, a, z + q);
        }
        if (u.pred_mode == 1) {
          if (u.skip) return fail(err, errn, "a skipped intra CU", k, a, z);
          if (u.chroma_dir != 36) {
            int ok = 0;
            for (int q = 0; q < 4; q++) { const int m[4] = { 0, 26, 10, 1 }; ok |= u.chroma_dir == (m[q] == u.luma_dir ? 34 : m[q]); }
            if (!ok) return fail(err, errn, "a chroma direction that is not among the allowed ones of its CU", k, a, z);
          }
        } else {
          if (u.skip && !(u.part_size == 0 && u.merge_flag && !((u.cbf[0] | u.cbf[1] | u.cbf[2]) & 1))) return fail(err, errn, "a skipped CU that is not a merged 2Nx2N CU without residual", k, a, z);
          for (int q = 0; q < np; q++) {
            const hop_cu_part& v = P[(size_t)a * 256 + z + q];
            if (v.merge_flag ? v.merge_idx > 4 : (v.mvp_idx < 0 || v.mvp_idx > 1)) return fail(err, errn, "merge index above 4 or predictor index outside 0..1", k, a, z + q);
            if (v.skip != u.skip) return fail(err, errn, "inconsistent skip flag inside a CU", k, a, z + q);
          }
        }
        z += np;
      }
    }
    if (levels) {
      const int32_t* Lv = levels + (size_t)k * n * 6144;
      for (size_t i = 0; i < (size_t)n * 6144; i++) if (Lv[i] > 32767 || Lv[i] < -32768) return fail(err, errn, "a level beyond 16 bits", k, (int)(i / 6144), (int)(i % 6144));
    }
    if (sao) {
      // What codeSAOBlkParam can carry (TEncSbac.cpp:2369-2480): the merge flags come from the LUMA entry whatever the slice flags say; type and edge class are coded once
      // for both chroma planes; of an edge offset only the magnitude is coded (the first two classes are >= 0, the last two <= 0: TEncSampleAdaptiveOffset.cpp:460-562).
      const int max_off = (1 << ((bit_depth < 10 ? bit_depth : 10) - 5)) - 1;
      for (int a = 0; a < n; a++) {
        const hop_sao_param* B = sao + ((size_t)k * n + a) * 3;
        if (B[0].mode < 0 || B[0].mode > 2) return fail(err, errn, "SAO mode out of range", k, a, 0);
        const bool merge = B[0].mode == 2;
        if (merge && (B[0].type < 0 || B[0].type > 1 || (B[0].type == 0 && a % wctu == 0) || (B[0].type == 1 && a < wctu))) return fail(err, errn, "SAO merge without its candidate", k, a, 0);
        for (int comp = 0; comp < 3; comp++) {
          const hop_sao_param& s = B[comp];
          if (!(comp ? p->sao_chroma : p->sao_luma)) { if (s.mode == 1) return fail(err, errn, "SAO offsets for a component the slice has switched off", k, a, comp); continue; }
          if (s.mode < 0 || s.mode > 2) return fail(err, errn, "SAO mode out of range", k, a, comp);
          if ((s.mode == 2) != merge || (merge && s.type != B[0].type)) return fail(err, errn, "SAO merge of one component only", k, a, comp);
          if (s.mode != 1) continue;
          if (s.type < 0 || s.type > 4 || (s.type == 4 && (s.aux < 0 || s.aux > 31))) return fail(err, errn, "SAO type or band position out of range", k, a, comp);
          if (s.type == 4) { for (int i = 0; i < 4; i++) { const int o = s.offset[(s.aux + i) & 31]; if (o > max_off || o < -max_off) return fail(err, errn, "SAO band offset out of range", k, a, comp); } }
          else for (int i = 0; i < 5; i++) {
            if (i == 2) continue;
            const int o = s.offset[i];
            if (i < 2 ? (o < 0 || o > max_off) : (o > 0 || o < -max_off)) return fail(err, errn, "SAO edge offset out of range or of the wrong sign", k, a, comp);
          }
        }
        if (!merge && p->sao_chroma) {
          const hop_sao_param &cb = B[1], &cr = B[2];
          if (cb.mode != cr.mode || (cb.mode == 1 && ((cb.type == 4) != (cr.type == 4) || (cb.type != 4 && cb.type != cr.type))))
            return fail(err, errn, "SAO type or edge class of Cr differs from Cb's (they are coded once)", k, a, 2);
        }
      }
    }
  }
  return HOP_OK;
}

int hop_slice_data_write_host(int pic_w, int pic_h, int bit_depth, const hop_slice_data_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao,
                              uint8_t* out, size_t out_capacity, uint32_t* substream_bytes, int32_t* n_substreams) {
  if (!levels || !substream_bytes || !n_substreams || (!out && out_capacity)) return HOP_ERR_ARG;
  char err[256];
  const int rc = hop_ent_check(pic_w, pic_h, bit_depth, 1, p, parts, levels, sao, err, sizeof(err));
  if (rc) return rc;
  std::vector<uint16_t> scans(4080 + 255);
  hop_rdoq_build_scans(scans.data());
  EntPic g;
  g.pic_w = pic_w; g.pic_h = pic_h; g.wctu = (pic_w + 63) / 64; g.hctu = (pic_h + 63) / 64;
  g.i_slice = p->slice_type == 2; g.sao_luma = p->sao_luma; g.sao_chroma = p->sao_chroma; g.sao_max_offset = (1 << ((bit_depth < 10 ? bit_depth : 10) - 5)) - 1;
  g.parts = parts; g.levels = levels; g.sao = sao; g.scans = scans.data();
  uint8_t init[EN_STATES];
  if (hop_ent_init_states(init, p->slice_type, p->qp)) return HOP_ERR_ARG;
  const int n_sub = p->wpp ? g.hctu : 1;
  std::vector<uint8_t> entry((size_t)g.hctu * EN_STATES);
  EntCoder k; memset(&k, 0, sizeof(k));
  if (p->wpp) en_context_pass(k, g, init, entry.data());
  size_t at = 0; int bad = 0;
  for (int s = 0; s < n_sub; s++) {
    const size_t room = at < out_capacity ? out_capacity - at : 0;
    en_code_substream(k, g, p->wpp ? &entry[(size_t)s * EN_STATES] : init, p->wpp ? s * g.wctu : 0, p->wpp ? g.wctu : g.wctu * g.hctu, out + (room ? at : 0),
                      (uint32_t)(room > 0xFFFFFFFFu ? 0xFFFFFFFFu : room));
    if (k.error) bad = 1;
    substream_bytes[s] = k.pos;
    at += k.pos;
  }
  if (bad) return HOP_ERR_ARG;                                            // a coded block without a level
  if (at > out_capacity) { *n_substreams = (int32_t)at; return HOP_ERR_ARG; }   // the size needed, in n_substreams' place
  *n_substreams = n_sub;
  return HOP_OK;
}

}  // extern "C"
