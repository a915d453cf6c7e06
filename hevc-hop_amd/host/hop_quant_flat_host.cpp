// hop_quant_flat_host.cpp -- host build of the leaf step's quantiser for units that do not use RDOQ (plain C++, no device code): csrc/k_quant_flat_dev.inl compiled by the
// host compiler with __device__ defined away.  hop_quant_flat_tu_host drives its two phases over `nlanes` emulated lanes, one phase after the other, the lanes of a phase
// in ascending or descending order.  Like hop_rdoq_tu_phased_host it is what the CPU tests drive (tests/test_quant_mode_cpu.py, tools/quant_flat_check.cpp), not a CPU
// path of the product.
#include <string.h>
#include <vector>
#include "../../include/hophip.h"

#define __device__
#define QF_HOST 1
#include "../csrc/k_quant_flat_dev.inl"

void hop_rdoq_build_scans(uint16_t* tabs /* 4080 + 255 entries */);   // host/hop_hostlogic.cpp

extern "C" int hop_quant_flat_tu_host(int bit_depth, int qp_scaled, int i_slice, int log2_size, int sign_hide, int scan_idx, const int32_t* coef, int32_t* level,
                                      uint32_t* abs_sum, int nlanes, int descending) {
  if (bit_depth < 8 || bit_depth > 12 || qp_scaled < 0 || qp_scaled > 87 || log2_size < 2 || log2_size > 5 || scan_idx < 0 || scan_idx > 2 || !coef || !level || !abs_sum ||
      nlanes < 1 || nlanes > 1024) return HOP_ERR_ARG;
  std::vector<uint16_t> tabs(4080 + 255);
  hop_rdoq_build_scans(tabs.data());
  // the scan of (scan_idx, log2_size): 1360 entries per scan index, the sizes one after the other (csrc/k_rdoq_dev.inl: rq_scan)
  const uint16_t* scan = tabs.data() + scan_idx * 1360 + (log2_size == 2 ? 0 : log2_size == 3 ? 16 : log2_size == 4 ? 80 : 336);
  const int N2 = 1 << (2 * log2_size);
  std::vector<int32_t> du((size_t)N2, (int32_t)0x5A5A5A5A);
  for (int i = 0; i < N2; i++) level[i] = (int32_t)0xA5A5A5A5;         // (every entry is written below)
  QfUnit u; u.log2_size = log2_size; u.qp_scaled = qp_scaled; u.bit_depth = bit_depth; u.i_slice = i_slice != 0; u.sign_hide = sign_hide != 0;
  QfPhase ph; ph.absSum = 0; ph.topSubset = -1;
#define LANES(call) for (int q = 0; q < nlanes; q++) { const int lane = descending ? nlanes - 1 - q : q; call; }
  LANES(quant_flat_levels(u, scan, coef, level, du.data(), &ph, lane, nlanes))
  LANES(quant_flat_sbh(u, scan, coef, level, du.data(), abs_sum, &ph, lane, nlanes))
#undef LANES
  return HOP_OK;
}
