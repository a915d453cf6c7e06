// hop_rdoq_host.cpp -- host builds of the leaf step's serial stages (plain C++, no device code): csrc/k_rdoq_dev.inl and csrc/k_estbits_dev.inl compiled by the host compiler
// with __device__ defined away.  hop_rdoq_tu_host is rdoq_tu, the one-lane body of k_rdoq and the yardstick; hop_rdoq_tu_phased_host drives the phased form the fused leaf
// bodies run (k_leaf_fused.inl) over `nlanes` emulated lanes, one phase after the other, the lanes of a phase in ascending or descending order; hop_estbits_setup_host /
// hop_estbits_fill_host are the one-lane and the cooperative bit-estimate table.  Like hop_slice_data_write_host they are what the CPU tests drive
// (tests/test_rdoq_phased_cpu.py, tools/rdoq_phased_check.cpp), not a CPU path of the product.
#include <math.h>
#include <string.h>
#include <vector>
#include "../../include/hophip.h"

#define __device__
#define RQ_HOST 1
#include "../csrc/k_rdoq_dev.inl"
#include "../csrc/k_estbits_dev.inl"

void hop_rdoq_build_scans(uint16_t* tabs /* 4080 + 255 entries */);   // host/hop_hostlogic.cpp

namespace {
const int32_t k_entropy_bits[128] = HOP_ENTROPY_BITS;

bool job_ok(const hop_rdoq_job* j) {
  return j && j->log2_size >= 2 && j->log2_size <= 5 && j->comp >= 0 && j->comp <= 2 && !(j->comp && j->log2_size == 5) && j->scan_idx >= 0 && j->scan_idx <= 2 &&
         j->bit_depth >= 8 && j->bit_depth <= 12 && j->qp_scaled >= 0 && j->qp_scaled <= 87 && j->tr_depth >= 0 && j->tr_depth <= 3 && j->lambda > 0;
}

struct Area {                                                          // what a leaf body gives the stage: scans, work area, group costs, phase record
  std::vector<uint16_t> tabs; std::vector<double> work; double cgSig[64]; uint16_t cgMask[64]; RqPhase ph; int plvl[1024]; double pcost[1024]; int pctx[1024];
  Area(int fill) : tabs(4080 + 255), work((size_t)1024 * RQ_WORK_PER_COEF / 8) {
    hop_rdoq_build_scans(tabs.data());
    memset(work.data(), fill, work.size() * 8); memset(cgSig, fill, sizeof(cgSig)); memset(cgMask, fill, sizeof(cgMask)); memset(&ph, fill, sizeof(ph)); memset(plvl, fill, sizeof(plvl)); memset(pcost, fill, sizeof(pcost)); memset(pctx, fill, sizeof(pctx));
  }
};

template <int LOG2> void phased(const hop_rdoq_job& jb, const hop_estbits* eb, Area& a, const int32_t* src, int32_t* dst, uint32_t* abs_sum, int nlanes, int descending) {
  const uint16_t* scan = rq_scan(a.tabs.data(), jb.scan_idx, LOG2); const uint16_t* scanCG = rq_scan_cg(a.tabs.data(), jb.scan_idx, LOG2);
  double* wd = a.work.data();
  // as the leaf bodies place them: a workgroup's 256 lanes prepare into arrays of their own, a wave (or one lane) into the work area
  RqPrep pp; pp.lvlD = a.plvl; pp.cost0 = a.pcost; pp.ctx = a.pctx;
  if (nlanes != 256) pp = rq_prep_in_work(wd, 1 << (2 * LOG2));
#define LANES(call) for (int q = 0; q < nlanes; q++) { const int lane = descending ? nlanes - 1 - q : q; call; }
  LANES(rdoq_prep_pos(jb, scan, src, pp, &a.ph, lane, nlanes))
  LANES(rdoq_prep_groups(jb, a.cgMask, pp, &a.ph, lane, nlanes))
  rdoq_serial<LOG2>(jb, eb, scan, scanCG, a.cgSig, a.cgMask, &a.ph, wd, pp);
  LANES(rdoq_finish_levels(jb, scan, src, wd, &a.ph, lane, nlanes))
  LANES(rdoq_finish_sbh(jb, scan, src, wd, &a.ph, lane, nlanes))
  LANES(rdoq_finish_scatter(jb, scan, dst, abs_sum, wd, &a.ph, lane, nlanes))
#undef LANES
}
}  // namespace

extern "C" {

int hop_rdoq_tu_host(const hop_rdoq_job* job, const hop_estbits* eb, const int32_t* src, int32_t* dst, uint32_t* abs_sum, int fill) {
  if (!job_ok(job) || !eb || !src || !dst || !abs_sum || fill < 0 || fill > 255) return HOP_ERR_ARG;
  Area a(fill);
  const hop_rdoq_job& jb = *job;
  const uint16_t* scan = rq_scan(a.tabs.data(), jb.scan_idx, jb.log2_size); const uint16_t* scanCG = rq_scan_cg(a.tabs.data(), jb.scan_idx, jb.log2_size);
  switch (jb.log2_size) {
    case 2: rdoq_tu<2>(jb, eb, scan, scanCG, a.cgSig, 1, src, dst, abs_sum, a.work.data(), 1, 0); break;
    case 3: rdoq_tu<3>(jb, eb, scan, scanCG, a.cgSig, 1, src, dst, abs_sum, a.work.data(), 1, 0); break;
    case 4: rdoq_tu<4>(jb, eb, scan, scanCG, a.cgSig, 1, src, dst, abs_sum, a.work.data(), 1, 0); break;
    default: rdoq_tu<5>(jb, eb, scan, scanCG, a.cgSig, 1, src, dst, abs_sum, a.work.data(), 1, 0); break;
  }
  return HOP_OK;
}

int hop_rdoq_tu_phased_host(const hop_rdoq_job* job, const hop_estbits* eb, const int32_t* src, int32_t* dst, uint32_t* abs_sum, int fill, int nlanes, int descending) {
  if (!job_ok(job) || !eb || !src || !dst || !abs_sum || fill < 0 || fill > 255 || nlanes < 1 || nlanes > 1024) return HOP_ERR_ARG;
  Area a(fill);
  switch (job->log2_size) {
    case 2: phased<2>(*job, eb, a, src, dst, abs_sum, nlanes, descending); break;
    case 3: phased<3>(*job, eb, a, src, dst, abs_sum, nlanes, descending); break;
    case 4: phased<4>(*job, eb, a, src, dst, abs_sum, nlanes, descending); break;
    default: phased<5>(*job, eb, a, src, dst, abs_sum, nlanes, descending); break;
  }
  return HOP_OK;
}

static bool tu_job_ok(const hop_tu_rd_job* j) { return j && j->log2_size >= 2 && j->log2_size <= 5 && j->comp >= 0 && j->comp <= 2 && !(j->comp && j->log2_size == 5); }

int hop_estbits_setup_host(const hop_tu_rd_job* job, const hop_cabac_ctx* ctx, hop_estbits* out) {
  if (!tu_job_ok(job) || !ctx || !out) return HOP_ERR_ARG;
  const int64_t off = 0; hop_rdoq_job rq; hop_coeff_bits_job cb;
  turd_setup_body(0, job, 1, ctx, &off, k_entropy_bits, out, &rq, &cb, ctx->state);
  return HOP_OK;
}

int hop_estbits_fill_host(const hop_tu_rd_job* job, const hop_cabac_ctx* ctx, hop_estbits* out, int nlanes, int descending) {
  if (!tu_job_ok(job) || !ctx || !out || nlanes < 1 || nlanes > 1024) return HOP_ERR_ARG;
  for (int q = 0; q < nlanes; q++) turd_estbits_fill(descending ? nlanes - 1 - q : q, nlanes, job->log2_size, job->comp, ctx->state, k_entropy_bits, out);
  return HOP_OK;
}

}  // extern "C"
