// hop_stream.cpp -- host side of hop_access_unit_write (plain C++, no device code): the layer around a picture's slice data that makes a stream a decoder opens --
// VPS / SPS / PPS, the slice header with its entry points, the decoded-picture-hash SEI, NAL framing with start codes, emulation prevention, MD5 and the checksum.
// Replaces: TEncCavlc::codeVPS / codeSPS / codePPS / codePTL / codeProfileTier / codeSliceHeader / codeTilesWPPEntryPoint (TLibEncoder/TEncCavlc.cpp:156-1070),
// writeNalUnitHeader, write and writeRBSPTrailingBits (TLibEncoder/NALwrite.cpp:67-170), the start codes of writeAnnexB (TLibEncoder/AnnexBwrite.h:46-78), SEIWriter for
// SEIDecodedPictureHash (TLibEncoder/SEIwrite.cpp:157-255) and calcMD5 / calcChecksum (TLibCommon/TComPicYuvMD5.cpp), in the configurations of hop_slice_data_write:
// whatever the option lists of the HOP all-intra and the plain intra configurations fix is a constant here, with the reference line that sets it.
// hop_access_unit_write_host, hop_parameter_sets_write and hop_rbsp_escape_host are whole entries; the device entry (csrc/k_stream.hip) shares the hop_strm_* pieces.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/hophip.h"

namespace {
// MSB-first bit writer (TComOutputBitstream::write, TLibCommon/TComBitStream.cpp:93-160) with the codes of SyntaxElementWriter (xWriteCode / xWriteUvlc / xWriteSvlc / xWriteFlag)
struct BitWriter {
  std::vector<uint8_t> bytes; uint32_t held; int n_held;
  BitWriter() : held(0), n_held(0) {}
  void code(uint32_t v, int n) {
    for (int i = n - 1; i >= 0; i--) {
      held = (held << 1) | ((v >> i) & 1u);
      if (++n_held == 8) { bytes.push_back((uint8_t)held); held = 0; n_held = 0; }
    }
  }
  void flag(int v) { code(v ? 1u : 0u, 1); }
  void ue(uint32_t v) {                                     // xWriteUvlc: the prefix of zeros, then v + 1
    int len = 0; const uint32_t t = v + 1;
    while ((t >> (len + 1)) != 0) len++;
    code(0, len); code(t, len + 1);
  }
  void se(int32_t v) { ue(v <= 0 ? (uint32_t)(-v) << 1 : ((uint32_t)v << 1) - 1); }   // xConvertToUInt
  void align_one() { while (n_held) code(1, 1); }           // writeAlignOne
  void trailing() { code(1, 1); while (n_held) code(0, 1); }   // writeRBSPTrailingBits / the slice header's byte alignment (TEncGOP.cpp:2810 writeByteAlignment): a 1, then zeros
};

// ---- MD5 (RFC 1321) ----
struct Md5 {
  uint32_t a, b, c, d; uint64_t n; uint8_t buf[64]; int fill;
  Md5() : a(0x67452301u), b(0xefcdab89u), c(0x98badcfeu), d(0x10325476u), n(0), fill(0) {}
  static uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
      0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
      0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
      0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
      0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391 };
    static const int S[64] = { 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20,
                               4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21 };
    uint32_t M[16];
    for (int i = 0; i < 16; i++) M[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    uint32_t A = a, B = b, C = c, D = d;
    for (int i = 0; i < 64; i++) {
      uint32_t F; int g;
      if (i < 16)      { F = (B & C) | (~B & D); g = i; }
      else if (i < 32) { F = (D & B) | (~D & C); g = (5 * i + 1) & 15; }
      else if (i < 48) { F = B ^ C ^ D;          g = (3 * i + 5) & 15; }
      else             { F = C ^ (B | ~D);       g = (7 * i) & 15; }
      F += A + K[i] + M[g];
      A = D; D = C; C = B; B += rol(F, S[i]);
    }
    a += A; b += B; c += C; d += D;
  }
  void update(const uint8_t* p, size_t len) {
    n += len;
    while (len) {
      if (fill == 0 && len >= 64) { block(p); p += 64; len -= 64; continue; }
      const size_t take = len < (size_t)(64 - fill) ? len : (size_t)(64 - fill);
      memcpy(buf + fill, p, take); fill += (int)take; p += take; len -= take;
      if (fill == 64) { block(buf); fill = 0; }
    }
  }
  void finish(uint8_t out[16]) {
    const uint64_t bits = n * 8;
    uint8_t pad[72]; memset(pad, 0, sizeof(pad)); pad[0] = 0x80;
    const int padlen = (fill < 56 ? 56 : 120) - fill;
    for (int i = 0; i < 8; i++) pad[padlen + i] = (uint8_t)(bits >> (8 * i));
    update(pad, (size_t)padlen + 8);
    const uint32_t v[4] = { a, b, c, d };
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
  }
};

// The sequential rule of write() (NALwrite.cpp:108-152): a counter of zeros, 03 in front of a byte <= 3 when the counter is 2, a final 03 behind a trailing 00.
// Returns the output length; stores below cap only.  emul: the insertions without the final 03 (TComOutputBitstream::countStartCodeEmulations, TComBitStream.cpp:186-216).
size_t escape(const uint8_t* in, size_t n, uint8_t* out, size_t cap, uint32_t* emul) {
  size_t at = 0; int zeros = 0; uint32_t cnt = 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t b = in[i];
    if (zeros == 2 && b <= 3) { if (at < cap) out[at] = 3; at++; zeros = 0; cnt++; }
    if (at < cap) out[at] = b;
    at++;
    zeros = b ? 0 : zeros + 1;
  }
  if (n && in[n - 1] == 0) { if (at < cap) out[at] = 3; at++; }
  if (emul) *emul = cnt;
  return at;
}

// a NAL unit behind its start code: zero_byte in front of the parameter sets and of the first unit of an access unit (AnnexBwrite.h:60); nal_unit_header with
// nuh_layer_id 0 and TemporalId 0 (writeNalUnitHeader, NALwrite.cpp:67-80)
void put_nal(std::vector<uint8_t>& s, int four, int type, const std::vector<uint8_t>& rbsp) {
  if (four) s.push_back(0);
  s.push_back(0); s.push_back(0); s.push_back(1);
  s.push_back((uint8_t)(type << 1)); s.push_back(1);
  std::vector<uint8_t> e(rbsp.size() + rbsp.size() / 2 + 2);
  const size_t n = escape(rbsp.data(), rbsp.size(), e.data(), e.size(), nullptr);
  s.insert(s.end(), e.begin(), e.begin() + n);
}

// general_profile_tier_level (codeProfileTier :977-995): --Profile none / main / main10 (TEncTop.cpp:636-653 sets the compatibility flag of the profile, and of
// main10 for main); Level none = 0, Tier main; the four source / constraint flags are 0 by default (ProgressiveSource ..., TAppEncCfg.cpp:381)
void profile_tier(BitWriter& w, const hop_stream_params* p, int bit_depth) {
  const int idc = !p->slice.plain_intra ? 0 : bit_depth == 8 ? 1 : 2;
  w.code(0, 2); w.flag(0); w.code(idc, 5);
  for (int j = 0; j < 32; j++) w.flag(j == idc || (idc == 1 && j == 2));
  w.flag(0); w.flag(0); w.flag(0); w.flag(0);
  w.code(0, 16); w.code(0, 16); w.code(0, 12);
}

void write_vps(BitWriter& w, const hop_stream_params* p, int bit_depth) {   // codeVPS :504-583
  w.code(0, 4); w.code(3, 2); w.code(0, 6);
  w.code(0, 3);                                            // one temporal layer (GOPSize 1)
  w.flag(1);                                               // vps_temporal_id_nesting_flag: one layer (TAppEncTop.cpp:79; the SPS: TEncTop.cpp:714)
  w.code(0xffff, 16);
  profile_tier(w, p, bit_depth); w.code(0, 8);             // codePTL: general_level_idc (Level none)
  w.flag(1);                                               // vps_sub_layer_ordering_info_present_flag
  w.ue(0); w.ue(0); w.ue(0);                               // max_dec_pic_buffering 1, no reordering, no latency limit: an intra-only sequence without GOP entries
  w.code(0, 6); w.ue(0);                                   // vps_max_nuh_reserved_zero_layer_id, vps_max_op_sets_minus1
  w.flag(0);                                               // vps_timing_info_present_flag
  // the fork's extension (IT_HOLOSS, :572-576): the flag is HoloscopicIntra, the micro-image size --MIsize (TAppEncTop.cpp:91-92; 0 where the plain configuration leaves both out)
  w.flag(!p->slice.plain_intra);
  w.align_one();
  w.ue(p->slice.plain_intra ? 0u : (uint32_t)p->slice.mi_size);
  w.flag(0);
  w.trailing();
}

void write_sps(BitWriter& w, int pic_w, int pic_h, int bit_depth, const hop_stream_params* p) {   // codeSPS :392-502
  w.code(0, 4); w.code(0, 3); w.flag(1);
  profile_tier(w, p, bit_depth); w.code(0, 8);
  w.ue(0); w.ue(1);                                        // sps id, chroma_format_idc 4:2:0
  w.ue(pic_w); w.ue(pic_h);                                // multiples of the minimum CU size 8: no padding
  w.flag(1); w.ue(0); w.ue(0); w.ue(0); w.ue(0);           // conformance_window_flag: TEncTop.cpp:661 copies the window the application set, all offsets 0 (setting it enables it, TComSlice.h:500-508)
  w.ue(bit_depth - 8); w.ue(bit_depth - 8);
  w.ue(4);                                                 // log2_max_pic_order_cnt_lsb_minus4: TComSPS::m_uiBitsForPOC = 8 (TComSlice.cpp:1645)
  w.flag(1); w.ue(0); w.ue(0); w.ue(0);
  w.ue(0); w.ue(3);                                        // MaxCUWidth 64, MaxPartitionDepth 4: coding blocks 8 .. 64
  w.ue(0); w.ue(3);                                        // QuadtreeTULog2MinSize 2, MaxSize 5
  w.ue(2); w.ue(2);                                        // QuadtreeTUMaxDepthInter / Intra 3
  w.flag(0);                                               // ScalingList 0
  w.flag(1);                                               // AMP 1
  w.flag(p->slice.sao_luma || p->slice.sao_chroma);        // SAO
  w.flag(0);                                               // PCMEnabledFlag 0
  w.ue(2);                                                 // num_short_term_ref_pic_sets: GOPSize + 1 (TEncTop.cpp:873 xInitRPS), both empty for IntraPeriod 1
  w.ue(0); w.ue(0);                                        // set 0: no negative, no positive pictures (codeShortTermRefPicSet :100-153)
  w.flag(0); w.ue(0); w.ue(0);                             // set 1: inter_ref_pic_set_prediction_flag 0, empty
  w.flag(0);                                               // long_term_ref_pics_present_flag
  w.flag(1);                                               // sps_temporal_mvp_enable_flag (TMVPMode 1 by default, TAppEncCfg.cpp:523; TEncGOP.cpp:871)
  w.flag(1);                                               // strong_intra_smoothing (default 1, TAppEncCfg.cpp:540)
  w.flag(0);                                               // vui_parameters_present_flag
  w.flag(0);
  w.trailing();
}

void write_pps(BitWriter& w, const hop_stream_params* p) {   // codePPS :156-231
  w.ue(0); w.ue(0); w.flag(0); w.flag(0); w.code(0, 3);
  w.flag(1);                                               // sign_data_hiding_flag (SBH 1 by default, TAppEncCfg.cpp:509)
  w.flag(0);                                               // cabac_init_present_flag
  w.ue(3); w.ue(3);                                        // num_ref_idx_l0 / l1_default_active_minus1: the most frequent count among the GOP entries, 4 without any (TEncTop.cpp:846-847)
  w.se(0);                                                 // init_qp_minus26: 0 without rate control
  w.flag(0);                                               // constrained_intra_pred_flag
  w.flag(1);                                               // TransformSkip 1
  w.flag(0);                                               // MaxDeltaQP 0: no cu_qp_delta
  w.se(0); w.se(0); w.flag(0);                             // no chroma QP offsets
  w.flag(0); w.flag(0);                                    // no weighted prediction
  w.flag(0);                                               // TransquantBypassEnableFlag 0
  w.flag(0);                                               // no tiles
  w.flag(p->slice.wpp);                                    // entropy_coding_sync_enabled_flag: WaveFrontSynchro
  w.flag(1);                                               // LFCrossSliceBoundaryFlag 1
  w.flag(0);                                               // DeblockingFilterControlPresent 0
  w.flag(0);                                               // ScalingList 0
  w.flag(0); w.ue(0); w.flag(0); w.flag(0);                // lists_modification_present_flag, log2_parallel_merge_level 2, no extensions
  w.trailing();
}

// SEIWriter::writeSEImessage (SEIwrite.cpp:157-196) for SEIDecodedPictureHash: payload type 132, size, hash_type = method - 1, the digests (:229-255)
void write_sei(BitWriter& w, int method, const uint8_t digest[3][16]) {
  const int per = method == 1 ? 16 : 4;
  w.code(132, 8); w.code(1 + 3 * per, 8); w.code(method - 1, 8);
  for (int c = 0; c < 3; c++) for (int i = 0; i < per; i++) w.code(digest[c][i], 8);
  w.trailing();
}
}  // namespace

extern "C" {
#define HIDDEN __attribute__((visibility("hidden")))

// internal: what the stream layer adds to the refusals of the slice-data writer
HIDDEN int hop_strm_check(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, char* err, size_t errn) {
  const char* what = nullptr;
  if (!p || pic_w <= 0 || pic_h <= 0) what = "bad argument";
  else if ((pic_w & 7) || (pic_h & 7)) what = "the picture's dimensions are no multiples of the minimum CU size 8";
  else if (pic_w > 65528 || pic_h > 65528) what = "picture too large";
  else if (bit_depth != 8 && bit_depth != 10) what = "bit depth other than 8 or 10";
  else if (p->hash == 2) what = "SEIDecodedPictureHash 2 (CRC) is not written";
  else if (p->hash != 0 && p->hash != 1 && p->hash != 3) what = "hash method out of range";
  else if (p->poc < 0 || (p->parameter_sets != 0 && p->parameter_sets != 1)) what = "poc or parameter_sets out of range";
  else if (p->slice.slice_type != 2 && p->slice.slice_type != 3) what = "only the I slice of the plain configurations and the ISS slice of the HOP configuration have a header here";
  else if ((p->slice.plain_intra != 0) != (p->slice.slice_type == 2)) what = "plain_intra goes with slice type I (2)";
  else if (!p->slice.plain_intra && bit_depth != 8) what = "the HOP configuration is 8 bit";
  else if (p->slice.mi_size < 0 || p->slice.qp < -6 * (bit_depth - 8) || p->slice.qp > 51 || (p->slice.wpp != 0 && p->slice.wpp != 1) ||
           (p->slice.sao_luma != 0 && p->slice.sao_luma != 1) || (p->slice.sao_chroma != 0 && p->slice.sao_chroma != 1)) what = "slice parameter out of range";
  if (what && err && errn) snprintf(err, errn, "hop_access_unit_write: %s", what);
  return what ? HOP_ERR_ARG : HOP_OK;
}

// internal: VPS, SPS, PPS with their four-byte start codes into s
HIDDEN void hop_strm_parameter_sets(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, std::vector<uint8_t>& s) {
  BitWriter v, q, r;
  write_vps(v, p, bit_depth); put_nal(s, 1, 32, v.bytes);
  write_sps(q, pic_w, pic_h, bit_depth, p); put_nal(s, 1, 33, q.bytes);
  write_pps(r, p); put_nal(s, 1, 34, r.bytes);
}

// internal: the two bytes of the NAL unit header and the slice segment header up to and including its byte alignment (codeSliceHeader :585-937, codeTilesWPPEntryPoint
// :1002-1070, TEncGOP.cpp:2810).  sub_bytes / sub_emul: per substream its length and the emulation-prevention bytes the NAL writer inserts into it alone (TEncGOP.cpp:1673).
HIDDEN void hop_strm_slice_header(int pic_w, int pic_h, const hop_stream_params* p, const uint32_t* sub_bytes, const uint32_t* sub_emul, int n_sub, std::vector<uint8_t>& s) {
  const hop_slice_data_params& sl = p->slice;
  BitWriter w;
  // nal_unit_type (TEncGOP::getNalUnitType, TEncGOP.cpp:2706): POC 0 is IDR_W_RADL (19); with DecodingRefreshType 0 no later picture is a random access point: TRAIL_R (1),
  // turned into TRAIL_N (0) because nothing refers to it -- except for an I slice at GOPSize 1 (TEncGOP.cpp:636-643), so only the HOP configuration's ISS slice becomes TRAIL_N
  w.code(0, 1); w.code(p->poc == 0 ? 19 : sl.plain_intra ? 1 : 0, 6); w.code(0, 6); w.code(1, 3);
  w.flag(1);                                               // first_slice_segment_in_pic_flag: SliceMode 0
  if (p->poc == 0) w.flag(0);                              // no_output_of_prior_pics_flag
  w.ue(0);
  w.ue(2);                                                 // slice_type: an ISS slice is written as I (:638-641)
  if (p->poc != 0) {
    w.code((uint32_t)p->poc & 255u, 8);                    // pic_order_cnt_lsb, 8 bits
    w.flag(1); w.code(0, 1);                               // short_term_ref_pic_set_sps_flag, set 0 of 2 (TEncGOP::selectReferencePictureSet: the GOP's entry)
    w.flag(sl.plain_intra);                                // slice_temporal_mvp_enable_flag: TMVPMode 1 enables it for every slice but the ISS slice, whose only reference is the picture itself (TEncGOP.cpp:861-872)
  }
  if (sl.sao_luma || sl.sao_chroma) { w.flag(sl.sao_luma); w.flag(sl.sao_chroma); }
  if (!sl.plain_intra) {                                   // ISS is not isIntra(): one reference picture (the picture itself) against the default 4, five merge candidates
    w.flag(1); w.ue(0);
    w.ue(0);
  }
  w.se(sl.qp - 26);
  w.flag(1);                                               // slice_loop_filter_across_slices_enabled_flag: the deblocking filter is on
  if (sl.wpp) {
    uint32_t max_off = 0;
    for (int i = 0; i + 1 < n_sub; i++) { const uint32_t o = sub_bytes[i] + sub_emul[i]; if (o > max_off) max_off = o; }
    uint32_t len_m1 = 0;
    while (len_m1 < 31 && max_off >= (1u << (len_m1 + 1))) len_m1++;
    w.ue(n_sub - 1);
    if (n_sub > 1) w.ue(len_m1);
    for (int i = 0; i + 1 < n_sub; i++) w.code(sub_bytes[i] + sub_emul[i] - 1, len_m1 + 1);
  }
  w.trailing();
  s.insert(s.end(), w.bytes.begin(), w.bytes.end());
  (void)pic_w; (void)pic_h;
}

// internal: the suffix SEI NAL unit (type 40) with its three-byte start code
HIDDEN void hop_strm_sei(int method, const uint8_t digest[3][16], std::vector<uint8_t>& s) {
  BitWriter w; write_sei(w, method, digest);
  put_nal(s, 0, 40, w.bytes);
}

// internal: the digest of one plane on the host (calcMD5 / calcChecksum): w x h samples at `stride`
HIDDEN void hop_strm_hash_plane(int method, int bit_depth, const int16_t* plane, int w, int h, size_t stride, uint8_t digest[16]) {
  memset(digest, 0, 16);
  if (method == 1) {
    Md5 m; std::vector<uint8_t> row((size_t)w * 2);
    for (int y = 0; y < h; y++) {
      const int16_t* r = plane + (size_t)y * stride;
      if (bit_depth <= 8) for (int x = 0; x < w; x++) row[x] = (uint8_t)r[x];
      else for (int x = 0; x < w; x++) { row[2 * x] = (uint8_t)r[x]; row[2 * x + 1] = (uint8_t)((uint16_t)r[x] >> 8); }
      m.update(row.data(), (size_t)w * (bit_depth <= 8 ? 1 : 2));
    }
    m.finish(digest);
  } else {
    uint32_t sum = 0;
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
      const uint32_t m = ((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff, v = (uint16_t)plane[(size_t)y * stride + x];   // UChar xor_mask (TComPicYuvMD5.cpp:144)
      sum += (v & 0xff) ^ m;
      if (bit_depth > 8) sum += (v >> 8) ^ m;
    }
    digest[0] = (uint8_t)(sum >> 24); digest[1] = (uint8_t)(sum >> 16); digest[2] = (uint8_t)(sum >> 8); digest[3] = (uint8_t)sum;
  }
}

int hop_rbsp_escape_host(const uint8_t* rbsp, const uint32_t* segment_bytes, int32_t n_segments, uint8_t* out, size_t cap, size_t* out_bytes, uint32_t* segment_emulations) {
  if (!rbsp || !segment_bytes || n_segments < 1 || !out_bytes || (!out && cap)) return HOP_ERR_ARG;
  size_t total = 0;
  for (int i = 0; i < n_segments; i++) { if (!segment_bytes[i]) return HOP_ERR_ARG; total += segment_bytes[i]; }
  if (segment_emulations) {
    size_t at = 0;
    for (int i = 0; i < n_segments; i++) { escape(rbsp + at, segment_bytes[i], nullptr, 0, &segment_emulations[i]); at += segment_bytes[i]; }
  }
  const size_t n = escape(rbsp, total, out, cap, nullptr);
  *out_bytes = n;
  return n > cap ? HOP_ERR_ARG : HOP_OK;
}

int hop_parameter_sets_write(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, uint8_t* out, size_t cap, size_t* bytes) {
  if (!bytes || (!out && cap)) return HOP_ERR_ARG;
  const int rc = hop_strm_check(pic_w, pic_h, bit_depth, p, nullptr, 0);
  if (rc) return rc;
  std::vector<uint8_t> s;
  hop_strm_parameter_sets(pic_w, pic_h, bit_depth, p, s);
  *bytes = s.size();
  if (s.size() > cap) return HOP_ERR_ARG;
  memcpy(out, s.data(), s.size());
  return HOP_OK;
}

int hop_access_unit_write_host(int pic_w, int pic_h, int bit_depth, const hop_stream_params* p, const hop_cu_part* parts, const int32_t* levels, const hop_sao_param* sao,
                               const int16_t* const rec[3], uint8_t* out, size_t cap, size_t* au_bytes) {
  if (!p || !parts || !levels || !au_bytes || (!out && cap)) return HOP_ERR_ARG;
  int rc = hop_strm_check(pic_w, pic_h, bit_depth, p, nullptr, 0);
  if (rc) return rc;
  if ((p->hash != 0) != (rec != nullptr) || (rec && (!rec[0] || !rec[1] || !rec[2]))) return HOP_ERR_ARG;
  const int hctu = (pic_h + 63) / 64;
  std::vector<uint32_t> sub(hctu), emul(hctu);
  std::vector<uint8_t> data((size_t)1 << 16);
  int32_t n_sub = 0;
  rc = hop_slice_data_write_host(pic_w, pic_h, bit_depth, &p->slice, parts, levels, sao, data.data(), data.size(), sub.data(), &n_sub);
  if (rc == HOP_ERR_ARG && n_sub > (int32_t)data.size()) {                // the size needed came back in n_substreams' place
    size_t need = 0; for (int i = 0; i < (p->slice.wpp ? hctu : 1); i++) need += sub[i];
    data.resize(need);
    rc = hop_slice_data_write_host(pic_w, pic_h, bit_depth, &p->slice, parts, levels, sao, data.data(), data.size(), sub.data(), &n_sub);
  }
  if (rc) return rc;
  size_t total = 0;
  for (int i = 0; i < n_sub; i++) { escape(data.data() + total, sub[i], nullptr, 0, &emul[i]); total += sub[i]; }
  std::vector<uint8_t> s;
  if (p->parameter_sets) hop_strm_parameter_sets(pic_w, pic_h, bit_depth, p, s);
  if (!p->parameter_sets) s.push_back(0);                                // the access unit's first NAL unit
  s.push_back(0); s.push_back(0); s.push_back(1);
  std::vector<uint8_t> nal;
  hop_strm_slice_header(pic_w, pic_h, p, sub.data(), emul.data(), n_sub, nal);
  nal.insert(nal.end(), data.begin(), data.begin() + total);
  std::vector<uint8_t> e(nal.size() + nal.size() / 2 + 2);
  const size_t n = escape(nal.data(), nal.size(), e.data(), e.size(), nullptr);   // (the header's two bytes end in 01: escaping them with the payload changes nothing)
  s.insert(s.end(), e.begin(), e.begin() + n);
  if (p->hash) {
    uint8_t digest[3][16];
    for (int c = 0; c < 3; c++) hop_strm_hash_plane(p->hash, bit_depth, rec[c], c ? pic_w / 2 : pic_w, c ? pic_h / 2 : pic_h, c ? pic_w / 2 : pic_w, digest[c]);
    hop_strm_sei(p->hash, digest, s);
  }
  *au_bytes = s.size();
  if (s.size() > cap) return HOP_ERR_ARG;                                 // the size needed is in au_bytes
  memcpy(out, s.data(), s.size());
  return HOP_OK;
}

}  // extern "C"
