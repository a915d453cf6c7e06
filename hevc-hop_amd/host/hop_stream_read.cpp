// hop_stream_read.cpp -- host side of hop_access_unit_read (plain C++, no device code): the mirror image of host/hop_stream.cpp.  An access unit's Annex B bytes are cut
// into NAL units, the NAL unit header, VPS / SPS / PPS, the slice header with its entry points and the decoded-picture-hash SEI are parsed, and the slice data behind the
// header is located -- in ESCAPED positions, which is what the entry points count.
// Replaces: byteStreamNALUnit (TLibDecoder/AnnexBread.cpp), read / readNalUnitHeader / convertPayloadToRBSP (TLibDecoder/NALread.cpp:52-145, the cabac_zero_words cut
// :79-94), TDecCavlc::parseVPS / parseSPS / parsePPS / parsePTL / parseProfileTier / parseSliceHeader (TLibDecoder/TDecCAVLC.cpp; the entry-point adjustment :1324-1355)
// and SEIReader::xReadSEImessage / xParseSEIDecodedPictureHash (TLibDecoder/SEIread.cpp), for the streams hop_access_unit_write writes: an element the writer emits as a
// constant must have that value, and the refusal names it.
// hop_access_unit_read_host, hop_rbsp_unescape_host and hop_annexb_access_unit are whole entries; the device entries (csrc/k_stream.hip) share hop_strm_read_syntax.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/hophip.h"
#include "hop_stream_read.h"

namespace {
struct Refusal { char* text; size_t n; bool set;
  void say(const char* fmt, ...) {
    if (set) return;
    set = true;
    if (!text || !n) return;
    const int k = snprintf(text, n, "hop_access_unit_read: ");
    if (k < 0 || (size_t)k >= n) return;
    va_list ap; va_start(ap, fmt); vsnprintf(text + k, n - k, fmt, ap); va_end(ap);
  }
};

// MSB-first bit reader over the ESCAPED bytes of a NAL unit (TComInputBitstream::read over convertPayloadToRBSP's result) with the codes of SyntaxElementParser
// (xReadCode / xReadUvlc / xReadSvlc / xReadFlag).  An emulation prevention byte is stepped over when the next byte is fetched, so `pos` is at every moment the escaped
// position behind the last byte that was read: the map back to escaped positions TDecCAVLC.cpp:1329-1335 rebuilds.  Reading past the end sets `over` and gives zeros.
struct BitReader {
  const uint8_t* p; size_t n, pos; int zeros, left; uint32_t cur; bool over;
  BitReader(const uint8_t* p_, size_t n_) : p(p_), n(n_), pos(0), zeros(0), left(0), cur(0), over(false) {}
  void fetch() {
    if (pos < n && zeros >= 2 && p[pos] == 3) { pos++; zeros = 0; }
    if (pos >= n) { over = true; cur = 0; left = 8; return; }
    cur = p[pos++]; left = 8;
    zeros = cur ? 0 : zeros + 1;
  }
  uint32_t bit() { if (!left) fetch(); left--; return (cur >> left) & 1u; }
  uint32_t code(int bits) { uint32_t v = 0; for (int i = 0; i < bits; i++) v = (v << 1) | bit(); return v; }
  uint32_t flag() { return bit(); }
  uint32_t ue() {                                              // xReadUvlc; a prefix beyond 31 zeros is no value of these streams
    int len = 0;
    while (!bit()) { if (++len > 31 || over) { over = true; return 0; } }
    return len ? ((1u << len) - 1u) + code(len) : 0u;
  }
  int32_t se() { const uint32_t v = ue(); return (v & 1u) ? (int32_t)((v + 1) >> 1) : -(int32_t)(v >> 1); }
  void skip(int bits) { for (int i = 0; i < bits; i++) bit(); }
  bool aligned() const { return left == 0; }
  bool at_end() {                                              // nothing but a final emulation prevention byte may follow
    size_t q = pos;
    if (q < n && zeros >= 2 && p[q] == 3) q++;
    return left == 0 && q >= n;
  }
};

struct Elem { BitReader& r; Refusal& e; const char* unit;
  void want(uint32_t got, uint32_t value, const char* name) { if (!r.over && got != value) e.say("%s: %s is %u, the writer writes %u", unit, name, got, value); }
  void flag(uint32_t value, const char* name) { want(r.flag(), value, name); }
  void code(int bits, uint32_t value, const char* name) { want(r.code(bits), value, name); }
  void ue(uint32_t value, const char* name) { want(r.ue(), value, name); }
  void se0(const char* name) { const int32_t v = r.se(); if (!r.over && v) e.say("%s: %s is %d, the writer writes 0", unit, name, v); }
  void trailing(bool to_end) {                                 // rbsp_trailing_bits / byte_alignment: a 1, then zeros
    if (!r.flag() && !r.over) e.say("%s: the stop bit is 0", unit);
    while (!r.aligned()) if (r.flag() && !r.over) { e.say("%s: an alignment bit is 1", unit); break; }
    if (r.over) e.say("%s ends inside an element", unit);
    else if (to_end && !r.at_end()) e.say("%s: bytes behind rbsp_trailing_bits", unit);
  }
};

struct Sets { int have_vps, have_sps, have_pps; int holo, mi, pic_w, pic_h, bit_depth, sao, wpp; };

// profile_tier_level with general_level_idc (parsePTL / parseProfileTier): read and ignored
void skip_ptl(BitReader& r) { r.skip(2 + 1 + 5 + 32 + 4 + 16 + 16 + 12 + 8); }

void read_vps(BitReader& r, Refusal& e, Sets& s) {             // parseVPS, the mirror of write_vps
  Elem x = { r, e, "VPS" };
  x.code(4, 0, "vps_video_parameter_set_id"); x.code(2, 3, "vps_reserved_three_2bits"); x.code(6, 0, "vps_max_layers_minus1");
  x.code(3, 0, "vps_max_sub_layers_minus1"); x.flag(1, "vps_temporal_id_nesting_flag"); x.code(16, 0xffff, "vps_reserved_ffff_16bits");
  skip_ptl(r);
  x.flag(1, "vps_sub_layer_ordering_info_present_flag");
  x.ue(0, "vps_max_dec_pic_buffering_minus1"); x.ue(0, "vps_num_reorder_pics"); x.ue(0, "vps_max_latency_increase_plus1");
  x.code(6, 0, "vps_max_nuh_reserved_zero_layer_id"); x.ue(0, "vps_max_op_sets_minus1"); x.flag(0, "vps_timing_info_present_flag");
  s.holo = (int)r.flag();                                      // vps_holo_extension_flag (IT_HOLOSS)
  while (!r.aligned()) if (!r.flag() && !r.over) { e.say("VPS: a vps_extension_alignment bit is 0"); break; }
  const uint32_t mi = r.ue();                                  // vps_holo_microimage_size
  if (mi > 65535) e.say("VPS: vps_holo_microimage_size %u", mi);
  s.mi = (int)mi;
  x.flag(0, "vps_extension2_flag");
  x.trailing(true);
  s.have_vps = 1;
}

void read_sps(BitReader& r, Refusal& e, Sets& s) {             // parseSPS, the mirror of write_sps
  Elem x = { r, e, "SPS" };
  x.code(4, 0, "sps_video_parameter_set_id"); x.code(3, 0, "sps_max_sub_layers_minus1"); x.flag(1, "sps_temporal_id_nesting_flag");
  skip_ptl(r);
  x.ue(0, "sps_seq_parameter_set_id"); x.ue(1, "chroma_format_idc");
  const uint32_t w = r.ue(), h = r.ue();
  x.flag(1, "conformance_window_flag");
  x.ue(0, "conf_win_left_offset"); x.ue(0, "conf_win_right_offset"); x.ue(0, "conf_win_top_offset"); x.ue(0, "conf_win_bottom_offset");
  const uint32_t bdy = r.ue(), bdc = r.ue();
  x.ue(4, "log2_max_pic_order_cnt_lsb_minus4");
  x.flag(1, "sps_sub_layer_ordering_info_present_flag");
  x.ue(0, "sps_max_dec_pic_buffering_minus1"); x.ue(0, "sps_num_reorder_pics"); x.ue(0, "sps_max_latency_increase_plus1");
  x.ue(0, "log2_min_coding_block_size_minus3"); x.ue(3, "log2_diff_max_min_coding_block_size");
  x.ue(0, "log2_min_transform_block_size_minus2"); x.ue(3, "log2_diff_max_min_transform_block_size");
  x.ue(2, "max_transform_hierarchy_depth_inter"); x.ue(2, "max_transform_hierarchy_depth_intra");
  x.flag(0, "scaling_list_enabled_flag"); x.flag(1, "amp_enabled_flag");
  s.sao = (int)r.flag();                                       // sample_adaptive_offset_enabled_flag
  x.flag(0, "pcm_enabled_flag");
  x.ue(2, "num_short_term_ref_pic_sets");
  x.ue(0, "num_negative_pics[0]"); x.ue(0, "num_positive_pics[0]");
  x.flag(0, "inter_ref_pic_set_prediction_flag[1]"); x.ue(0, "num_negative_pics[1]"); x.ue(0, "num_positive_pics[1]");
  x.flag(0, "long_term_ref_pics_present_flag"); x.flag(1, "sps_temporal_mvp_enable_flag"); x.flag(1, "strong_intra_smoothing_enable_flag");
  x.flag(0, "vui_parameters_present_flag"); x.flag(0, "sps_extension_flag");
  x.trailing(true);
  if (!r.over) {
    if (w == 0 || h == 0 || (w & 7) || (h & 7) || w > 65528 || h > 65528) e.say("SPS: a picture of %u x %u (multiples of 8 up to 65528)", w, h);
    if (bdy != bdc || (bdy != 0 && bdy != 2)) e.say("SPS: bit depths %u / %u (8 or 10, luma and chroma alike)", bdy + 8, bdc + 8);
  }
  s.pic_w = (int)w; s.pic_h = (int)h; s.bit_depth = (int)bdy + 8;
  s.have_sps = 1;
}

void read_pps(BitReader& r, Refusal& e, Sets& s) {             // parsePPS, the mirror of write_pps
  Elem x = { r, e, "PPS" };
  x.ue(0, "pps_pic_parameter_set_id"); x.ue(0, "pps_seq_parameter_set_id"); x.flag(0, "dependent_slice_segments_enabled_flag");
  x.flag(0, "output_flag_present_flag"); x.code(3, 0, "num_extra_slice_header_bits"); x.flag(1, "sign_data_hiding_flag"); x.flag(0, "cabac_init_present_flag");
  x.ue(3, "num_ref_idx_l0_default_active_minus1"); x.ue(3, "num_ref_idx_l1_default_active_minus1");
  x.se0("init_qp_minus26");
  x.flag(0, "constrained_intra_pred_flag"); x.flag(1, "transform_skip_enabled_flag"); x.flag(0, "cu_qp_delta_enabled_flag");
  x.se0("pps_cb_qp_offset"); x.se0("pps_cr_qp_offset"); x.flag(0, "pps_slice_chroma_qp_offsets_present_flag");
  x.flag(0, "weighted_pred_flag"); x.flag(0, "weighted_bipred_flag"); x.flag(0, "transquant_bypass_enable_flag"); x.flag(0, "tiles_enabled_flag");
  s.wpp = (int)r.flag();                                       // entropy_coding_sync_enabled_flag
  x.flag(1, "loop_filter_across_slices_enabled_flag"); x.flag(0, "deblocking_filter_control_present_flag"); x.flag(0, "pps_scaling_list_data_present_flag");
  x.flag(0, "lists_modification_present_flag"); x.ue(0, "log2_parallel_merge_level_minus2"); x.flag(0, "slice_segment_header_extension_present_flag");
  x.flag(0, "pps_extension_flag");
  x.trailing(true);
  s.have_pps = 1;
}

// sei_rbsp (xReadSEImessage): every message's type and size as runs of ff; the decoded picture hash (132, suffix) is read, the others are stepped over
void read_sei(BitReader& r, Refusal& e, int nal_type, int* hash, uint8_t digest[3][16]) {
  for (int guard = 0; guard < 4096 && !r.over && !e.set; guard++) {
    uint32_t type = 0, size = 0, b;
    do { b = r.code(8); type += b; } while (b == 0xff && !r.over && type < 65536);
    do { b = r.code(8); size += b; } while (b == 0xff && !r.over && size < (1u << 24));
    if (r.over) break;
    if (type == 132 && nal_type == 40) {
      const uint32_t method = r.code(8), per = method == 0 ? 16 : method == 1 ? 2 : 4;
      if (r.over) break;
      if (method > 2) { e.say("SEI: hash_type %u", method); return; }
      if (size != 1 + 3 * per) { e.say("SEI: a decoded picture hash of %u bytes, hash_type %u takes %u", size, method, 1 + 3 * per); return; }
      if (*hash) { e.say("SEI: more than one decoded picture hash"); return; }
      *hash = (int)method + 1;
      for (int c = 0; c < 3; c++) for (uint32_t i = 0; i < per; i++) digest[c][i] = (uint8_t)r.code(8);
    } else {
      for (uint32_t i = 0; i < size && !r.over; i++) r.code(8);
    }
    if (r.over) break;
    // more_rbsp_data: anything but the trailing bits
    BitReader t = r;
    if (t.code(8) == 0x80 && !t.over && t.at_end()) { r = t; return; }
  }
  if (!e.set) e.say("SEI ends inside an element");
}

struct Unit { size_t at, len; int type; };

// the NAL units of an Annex B stream: behind every 00 00 01, up to the next one; the zero bytes in front of a start code (its zero_byte, leading and trailing
// zero_8bits) belong to no unit -- a NAL unit never ends in 00
void find_units(const uint8_t* d, size_t n, std::vector<Unit>& out, std::vector<size_t>* code_at) {
  size_t i = 0;
  std::vector<size_t> starts;
  while (i + 3 <= n) {
    if (d[i] == 0 && d[i + 1] == 0 && d[i + 2] == 1) { starts.push_back(i); i += 3; }
    else i++;
  }
  for (size_t k = 0; k < starts.size(); k++) {
    Unit u; u.at = starts[k] + 3;
    size_t end = k + 1 < starts.size() ? starts[k + 1] : n;
    while (end > u.at && d[end - 1] == 0) end--;
    u.len = end - u.at;
    u.type = u.len ? (d[u.at] >> 1) & 0x3f : -1;
    out.push_back(u);
    if (code_at) { size_t s = starts[k]; const size_t floor = k ? out[k - 1].at + out[k - 1].len : 0; while (s > floor && d[s - 1] == 0) s--; code_at->push_back(s); }
  }
}

// the sequential rule (convertPayloadToRBSP, NALread.cpp:59-76): a counter of zeros, an 03 dropped when the counter is 2 or more.  in: `lookback` bytes that only feed
// the counter, then the segments.  Returns the output length; stores below cap only.
size_t unescape(const uint8_t* in, int lookback, const uint32_t* seg, int n_seg, uint8_t* out, size_t cap, uint32_t* seg_rbsp, uint32_t* viol) {
  int zeros = 0;
  for (int i = 0; i < lookback; i++) zeros = in[i] ? 0 : zeros + 1;
  const uint8_t* p = in + lookback;
  size_t at = 0, i = 0; uint32_t bad = 0; bool dropped = false;
  for (int s = 0; s < n_seg; s++) {
    uint32_t kept = 0;
    for (uint32_t k = 0; k < seg[s]; k++, i++) {
      const uint8_t b = p[i];
      if (dropped && b > 3) bad++;
      dropped = false;
      if (zeros >= 2 && b == 3) { zeros = 0; dropped = true; continue; }
      if (zeros >= 2 && b <= 2) bad++;
      if (at < cap) out[at] = b;
      at++; kept++;
      zeros = b ? 0 : zeros + 1;
    }
    if (seg_rbsp) seg_rbsp[s] = kept;
  }
  if (viol) *viol = bad;
  return at;
}
}  // namespace

extern "C" {
#define HIDDEN __attribute__((visibility("hidden")))

// internal: everything of an access unit but its slice data -- the units, the parameter sets (or `active`), the slice header, the SEI; where the slice data lies and how
// the entry points cut it, in escaped bytes.  dims: the context's {pic_w, pic_h, bit_depth} to compare with, or NULL.
HIDDEN int hop_strm_read_syntax(const uint8_t* au, size_t n, const hop_stream_info* active, const int* dims, int max_substreams, hop_strm_au* out, char* err, size_t errn) {
  Refusal e = { err, errn, false };
  if (err && errn) err[0] = 0;
  std::vector<Unit> units;
  find_units(au, n, units, nullptr);
  Sets s; memset(&s, 0, sizeof(s));
  int vcl = -1, hash = 0;
  memset(out->digest, 0, sizeof(out->digest));
  for (size_t k = 0; k < units.size() && !e.set; k++) {
    const Unit& u = units[k];
    if (u.len < 2) { e.say("NAL unit %zu is shorter than its header", k); break; }
    BitReader r(au + u.at, u.len);
    Elem x = { r, e, "NAL unit header" };
    x.flag(0, "forbidden_zero_bit"); r.skip(6); x.code(6, 0, "nuh_layer_id"); x.code(3, 1, "nuh_temporal_id_plus1");
    if (e.set) break;
    if (u.type < 32) {
      if (vcl >= 0) { e.say("more than one VCL NAL unit"); break; }
      if (u.type != 19 && u.type != 0 && u.type != 1) { e.say("nal_unit_type %d: the writer writes 19 (IDR_W_RADL), 0 (TRAIL_N) and 1 (TRAIL_R)", u.type); break; }
      vcl = (int)k;
    } else if (u.type >= 32 && u.type <= 34) {
      if (vcl >= 0) { e.say("a parameter set behind the VCL NAL unit"); break; }
      if (u.type == 32) read_vps(r, e, s); else if (u.type == 33) read_sps(r, e, s); else read_pps(r, e, s);
    } else if (u.type == 39 || u.type == 40) {
      if (u.type == 40 && vcl < 0) { e.say("a suffix SEI in front of the VCL NAL unit"); break; }
      read_sei(r, e, u.type, &hash, out->digest);
    }                                                         // anything else (access unit delimiter, filler data, ...) carries nothing the decoder needs
  }
  if (e.set) return HOP_ERR_ARG;
  if (vcl < 0) { e.say("no VCL NAL unit"); return HOP_ERR_ARG; }
  const int n_sets = s.have_vps + s.have_sps + s.have_pps;
  if (n_sets != 0 && n_sets != 3) { e.say("parameter sets incomplete: VPS %d, SPS %d, PPS %d", s.have_vps, s.have_sps, s.have_pps); return HOP_ERR_ARG; }
  if (active) {
    const hop_slice_data_params& a = active->params.slice;
    const int a_sao = a.sao_luma || a.sao_chroma;
    if (n_sets) {
      const struct { const char* name; int got, want; } f[7] = { { "pic_w", s.pic_w, active->pic_w }, { "pic_h", s.pic_h, active->pic_h }, { "bit_depth", s.bit_depth, active->bit_depth },
        { "plain_intra", !s.holo, a.plain_intra != 0 }, { "mi_size", s.mi, a.mi_size }, { "wpp", s.wpp, a.wpp }, { "the SAO flag", s.sao, a_sao } };
      for (int k = 0; k < 7; k++) if (f[k].got != f[k].want) { e.say("the parameter sets contradict `active`: %s %d, `active` has %d", f[k].name, f[k].got, f[k].want); return HOP_ERR_ARG; }
    }
    if (!n_sets) { s.pic_w = active->pic_w; s.pic_h = active->pic_h; s.bit_depth = active->bit_depth; s.holo = !a.plain_intra; s.mi = a.mi_size; s.wpp = a.wpp; s.sao = a_sao; }
  } else if (!n_sets) { e.say("the access unit carries no parameter sets and `active` is NULL"); return HOP_ERR_ARG; }
  if (s.pic_w <= 0 || s.pic_h <= 0 || (s.pic_w & 7) || (s.pic_h & 7) || s.pic_w > 65528 || s.pic_h > 65528 || (s.bit_depth != 8 && s.bit_depth != 10) || (s.holo != 0 && s.holo != 1) ||
      (s.wpp != 0 && s.wpp != 1) || s.mi < 0) { e.say("`active` is no info of this reader"); return HOP_ERR_ARG; }
  if (s.holo && s.bit_depth != 8) { e.say("the HOP configuration is 8 bit, the SPS says %d", s.bit_depth); return HOP_ERR_ARG; }
  if (dims && (dims[0] != s.pic_w || dims[1] != s.pic_h || dims[2] != s.bit_depth)) {
    e.say("a picture of %d x %d at %d bit, the context's is %d x %d at %d bit", s.pic_w, s.pic_h, s.bit_depth, dims[0], dims[1], dims[2]); return HOP_ERR_ARG;
  }
  // the slice NAL unit: trailing zero bytes are cut (cabac_zero_words, NALread.cpp:79-94) -- in the escaped domain, where a zero word ends in its own 03
  const Unit& u = units[vcl];
  size_t len = u.len;
  const uint8_t* p = au + u.at;
  while (len > 2) {
    if (p[len - 1] == 0) len--;
    else if (p[len - 1] == 3 && len >= 3 && p[len - 2] == 0 && p[len - 3] == 0) len--;
    else break;
  }
  BitReader r(p, len);
  Elem x = { r, e, "slice header" };
  r.skip(16);
  const int idr = u.type == 19;
  x.flag(1, "first_slice_segment_in_pic_flag");
  if (idr) x.flag(0, "no_output_of_prior_pics_flag");
  x.ue(0, "slice_pic_parameter_set_id"); x.ue(2, "slice_type");
  int poc = 0;
  if (!idr) {
    if (u.type != (s.holo ? 0 : 1)) e.say("nal_unit_type %d: a later picture is %s here", u.type, s.holo ? "TRAIL_N (0) with the HOP extension" : "TRAIL_R (1) without it");
    poc = (int)r.code(8);
    x.flag(1, "short_term_ref_pic_set_sps_flag"); x.code(1, 0, "short_term_ref_pic_set_idx"); x.flag(s.holo ? 0 : 1, "slice_temporal_mvp_enable_flag");
  }
  int sao_luma = 0, sao_chroma = 0;
  if (s.sao) {
    sao_luma = (int)r.flag(); sao_chroma = (int)r.flag();
    if (!sao_luma && !sao_chroma && !r.over) e.say("slice header: both SAO flags 0 under an SPS that enables SAO; the writer writes no such stream");
  }
  if (s.holo) { x.flag(1, "num_ref_idx_active_override_flag"); x.ue(0, "num_ref_idx_l0_active_minus1"); x.ue(0, "five_minus_max_num_merge_cand"); }
  const int qp = 26 + r.se();
  x.flag(1, "slice_loop_filter_across_slices_enabled_flag");
  const int hctu = (s.pic_h + 63) / 64;
  out->seg.clear();
  if (s.wpp && !e.set && !r.over) {
    const uint32_t n_entry = r.ue();
    if (!r.over && (int64_t)n_entry + 1 != hctu) e.say("%u substreams, the picture has %d CTU rows", n_entry + 1, hctu);
    else if (!r.over && (int64_t)n_entry + 1 > max_substreams) e.say("%u substreams, max_substreams is %d", n_entry + 1, max_substreams);
    else if (n_entry && !r.over) {
      const uint32_t len_m1 = r.ue();
      if (len_m1 > 31) e.say("slice header: offset_len_minus1 %u", len_m1);
      for (uint32_t i = 0; i < n_entry && !r.over && !e.set; i++) {
        const uint32_t v = r.code((int)len_m1 + 1);
        if (v == 0xffffffffu) { e.say("slice header: entry point %u overflows", i); break; }
        out->seg.push_back(v + 1);
      }
    }
  }
  if (!e.set) x.trailing(false);
  if (!e.set && r.over) e.say("slice header ends inside an element");
  if (e.set) return HOP_ERR_ARG;
  if (qp < -6 * (s.bit_depth - 8) || qp > 51) { e.say("slice header: a slice QP of %d", qp); return HOP_ERR_ARG; }
  if (max_substreams < 1) { e.say("1 substream, max_substreams is %d", max_substreams); return HOP_ERR_ARG; }
  const size_t head = r.pos;                                   // behind the header's last byte; an 03 that follows belongs to the first substream (:1346)
  size_t sum = 0;
  for (size_t i = 0; i < out->seg.size(); i++) { sum += out->seg[i]; if (sum >= len - head || sum < out->seg[i]) { e.say("the entry points sum past the payload (%zu bytes)", len - head); return HOP_ERR_ARG; } }
  if (head >= len) { e.say("an empty substream: no slice data behind the slice header"); return HOP_ERR_ARG; }
  if (len - head - sum > 0x7fffffffu) { e.say("more than 2^31 - 1 bytes of slice data"); return HOP_ERR_ARG; }
  out->seg.push_back((uint32_t)(len - head - sum));
  hop_stream_info& o = out->info;
  memset(&o, 0, sizeof(o));
  o.pic_w = s.pic_w; o.pic_h = s.pic_h; o.bit_depth = s.bit_depth;
  o.params.slice.qp = qp; o.params.slice.slice_type = s.holo ? 3 : 2; o.params.slice.wpp = s.wpp; o.params.slice.plain_intra = !s.holo;
  o.params.slice.sao_luma = sao_luma; o.params.slice.sao_chroma = sao_chroma; o.params.slice.mi_size = s.mi;
  o.params.poc = poc; o.params.parameter_sets = n_sets ? 1 : 0; o.params.hash = hash;
  o.nal_type = u.type; o.n_substreams = (int32_t)out->seg.size(); o.header_bytes = (int32_t)head;
  out->nal_at = u.at; out->nal_len = len;
  return HOP_OK;
}

// internal: what both entries check once the substreams' RBSP sizes are known
HIDDEN int hop_strm_read_sizes(const uint32_t* rbsp_bytes, int n_sub, uint32_t violations, char* err, size_t errn) {
  Refusal e = { err, errn, false };
  if (violations) { e.say("%u positions of the slice data break emulation prevention (a byte <= 2 behind 00 00, or a byte > 3 behind a removed 03)", violations); return HOP_ERR_ARG; }
  for (int i = 0; i < n_sub; i++) if (!rbsp_bytes[i]) { e.say("substream %d is empty", i); return HOP_ERR_ARG; }
  return HOP_OK;
}

int hop_rbsp_unescape_host(const uint8_t* escaped, const uint32_t* segment_bytes, int32_t n_segments, int32_t lookback, uint8_t* out, size_t cap, size_t* out_bytes,
                           uint32_t* segment_rbsp_bytes, uint32_t* violations) {
  if (!escaped || !segment_bytes || n_segments < 1 || lookback < 0 || lookback > 2 || !out_bytes || (!out && cap)) return HOP_ERR_ARG;
  size_t total = 0;
  for (int i = 0; i < n_segments; i++) { if (!segment_bytes[i]) return HOP_ERR_ARG; total += segment_bytes[i]; if (total > 0x7fffffffu) return HOP_ERR_ARG; }
  const size_t n = unescape(escaped, lookback, segment_bytes, n_segments, out, cap, segment_rbsp_bytes, violations);
  *out_bytes = n;
  return n > cap ? HOP_ERR_ARG : HOP_OK;
}

int hop_access_unit_read_host(const uint8_t* au, size_t au_bytes, const hop_stream_info* active, hop_stream_info* info, uint8_t* data, size_t cap, size_t* data_bytes,
                              uint32_t* substream_bytes, int32_t max_substreams, uint8_t (*digest)[16]) {
  if (!au || !info || !data_bytes || !substream_bytes || !digest || (!data && cap)) return HOP_ERR_ARG;
  hop_strm_au a;
  int rc = hop_strm_read_syntax(au, au_bytes, active, nullptr, max_substreams, &a, nullptr, 0);
  if (rc) return rc;
  const int n_sub = (int)a.seg.size(), back = a.info.header_bytes < 2 ? a.info.header_bytes : 2;
  uint32_t viol = 0;
  const size_t n = unescape(au + a.nal_at + a.info.header_bytes - back, back, a.seg.data(), n_sub, data, cap, substream_bytes, &viol);
  rc = hop_strm_read_sizes(substream_bytes, n_sub, viol, nullptr, 0);
  if (rc) return rc;
  *data_bytes = n;
  *info = a.info;
  memcpy(digest, a.digest, sizeof(a.digest));
  return n > cap ? HOP_ERR_ARG : HOP_OK;                       // the size needed is in data_bytes
}

int hop_annexb_access_unit(const uint8_t* stream, size_t bytes, size_t* au_bytes) {
  if (!stream || !au_bytes) return HOP_ERR_ARG;
  std::vector<Unit> units; std::vector<size_t> code_at;
  find_units(stream, bytes, units, &code_at);
  if (units.empty()) return HOP_ERR_ARG;
  bool vcl = false;
  for (size_t k = 0; k < units.size(); k++) {
    if (vcl && units[k].type != 40) { *au_bytes = code_at[k]; return HOP_OK; }
    if (units[k].type >= 0 && units[k].type < 32) vcl = true;
  }
  *au_bytes = bytes;
  return HOP_OK;
}

}  // extern "C"
