// hop_stream_read.h -- what host/hop_stream_read.cpp shares with the device entries of csrc/k_stream.hip (internal, not part of the ABI)
#ifndef HOP_STREAM_READ_H
#define HOP_STREAM_READ_H
#include <vector>
#include "../../include/hophip.h"

// an access unit after the host pass: the info, the SEI's digests, the VCL NAL unit au[nal_at .. nal_at + nal_len) behind its start code with the trailing zero bytes
// cut, and the substreams' sizes in ESCAPED bytes from au[nal_at + info.header_bytes] on (the entry points, then what remains)
struct hop_strm_au {
  hop_stream_info info;
  uint8_t digest[3][16];
  size_t nal_at, nal_len;
  std::vector<uint32_t> seg;
};

extern "C" {
__attribute__((visibility("hidden"))) int hop_strm_read_syntax(const uint8_t* au, size_t n, const hop_stream_info* active, const int* dims, int max_substreams, hop_strm_au* out, char* err, size_t errn);
__attribute__((visibility("hidden"))) int hop_strm_read_sizes(const uint32_t* rbsp_bytes, int n_sub, uint32_t violations, char* err, size_t errn);
}
#endif
