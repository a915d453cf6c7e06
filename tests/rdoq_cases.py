"""Generated transform units for the leaf step's serial stages (tests/test_rdoq_phased_cpu.py, tools/rdoq_phased_check.cpp through the file write_case_file makes,
tests/test_gpu_leaf_phases.py): for every unit size, component class, scan the size can have and sign_hide 0 / 1 the families

  zero       every coefficient zero (no last significant position: the serial lane has nothing to do)
  first      one level at scan position 0
  last       one level at the last position of the last coefficient group
  saturated  every position at +-32767 (the quantiser's cap, levels at the 16-bit bound that sign hiding must not cross)
  dense      a level almost everywhere (every group coded, Rice parameter and context sets moving)
  sparse     a few levels, most groups empty
  lone<v>    one coefficient of magnitude v in a middle group below one weak coefficient (candidate level 1) in the last group, v swept from below one quantiser step
             to four: along the sweep the middle group -- the only one with a level once the last-position pass has dropped the top coefficient -- goes from dropped
             by the per-coefficient decision over zeroed by the group decision (TComTrQuant.cpp:1700-1760) to kept

The bit-estimate table of a unit is hop_estbits_setup_host's for the unit's size and component from context states hop_cabac_init makes (slice type and QP vary)."""
import ctypes

import numpy as np

SIZES = [(2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1), (5, 0)]          # (log2, component class): the reference has no chroma 32x32
FILE_MAGIC = 0x51445248


def scans_of(log2):
    return (0, 1, 2) if log2 <= 3 else (0,)


def diag_scan(log2):
    """the scan position -> raster position table of the up-right diagonal scan in 4x4 groups (TComRom.cpp:355-481), for placing a coefficient at a scan position"""
    def diag(n):
        out = []
        for s in range(2 * n - 1):
            for y in range(min(s, n - 1), -1, -1):
                x = s - y
                if x < n: out.append((x, y))
        return out
    n = 1 << log2
    if log2 == 2: return [y * n + x for x, y in diag(4)]
    pos = []
    for gx, gy in diag(n // 4):
        pos += [(4 * gy + y) * n + 4 * gx + x for x, y in diag(4)]
    return pos


def bind(L):
    L.hop_cabac_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.hop_estbits_setup_host.argtypes = [ctypes.c_void_p] * 3
    L.hop_estbits_fill_host.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2
    L.hop_rdoq_tu_host.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int]
    L.hop_rdoq_tu_phased_host.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3
    return L


def table_for(L, hp, log2, comp, slice_type, qp, states=None):
    job = np.zeros(1, hp.TU_RD_JOB_DTYPE); job["log2_size"], job["comp"] = log2, comp
    ctx = np.zeros(hp.CABAC_CTX_BYTES, np.uint8)
    if states is None: assert L.hop_cabac_init(ctx.ctypes.data, slice_type, qp) == 0
    else: ctx[:] = states
    eb = np.zeros(hp.ESTBITS_INTS, np.int32)
    assert L.hop_estbits_setup_host(job.ctypes.data, ctx.ctypes.data, eb.ctypes.data) == 0
    return eb


def rdoq_job(hp, c):
    j = np.zeros(1, hp.RDOQ_JOB_DTYPE)
    j["log2_size"], j["comp"], j["is_intra"], j["scan_idx"], j["tr_depth"], j["qp_scaled"] = c["log2"], c["comp"], c["intra"], c["scan"], c["tr"], c["qp"]
    j["bit_depth"], j["sign_hide"], j["lambda"] = c["bd"], c["sh"], c["lam"]
    return j


def unit_cases(L, hp):
    """the generated units, each a dict like goldutil.encoder_rdoq_calls' (without `out`) plus `name`"""
    rng = np.random.default_rng(20261020)
    out = []
    for log2, comp in SIZES:
        n = 1 << (2 * log2); pos = diag_scan(log2)
        for scan in scans_of(log2):
            for sh in (0, 1):
                def unit(name, src, qp=None):
                    qp = int(rng.integers(18, 42)) if qp is None else qp
                    intra = 1 if scan else int(rng.integers(0, 2))
                    c = dict(name="%dx%d %s scan %d sh %d %s" % (1 << log2, 1 << log2, "chroma" if comp else "luma", scan, sh, name), log2=log2, comp=comp, intra=intra,
                             scan=scan, tr=int(rng.integers(0, 3)), qp=qp, bd=8, sh=sh, lam=0.57 * 2.0 ** ((qp - 12) / 3.0) * float(rng.choice([1.0, 0.8])),
                             src=np.ascontiguousarray(src, np.int32))
                    c["eb"] = table_for(L, hp, log2, comp, int(rng.integers(0, 5)), qp)
                    out.append(c)
                z = np.zeros(n, np.int32)
                unit("zero", z)
                a = z.copy(); a[pos[0]] = int(rng.choice([-1, 1])) * int(rng.integers(300, 3000)); unit("first", a)
                a = z.copy(); a[pos[n - 1]] = int(rng.choice([-1, 1])) * int(rng.integers(300, 3000)); unit("last", a)
                unit("saturated", rng.choice([-32767, 32767], n))
                unit("dense", np.rint(rng.laplace(0, 600, n)) * (rng.random(n) < 0.9))
                a = np.rint(rng.laplace(0, 400, n)) * (rng.random(n) < (0.3 if log2 == 2 else 0.04)); unit("sparse", a)
                if log2 >= 3:
                    groups = n // 16
                    for qp in (24, 31):
                        # |coefficient| of a candidate level 1: 2^qBits / quantiser scale (csrc/k_rdoq_dev.inl: qBits = 14 + qp / 6 + 15 - 8 - log2)
                        one = 2.0 ** (29 + qp // 6 - 8 - log2) / (26214, 23302, 20560, 18396, 16384, 14564)[qp % 6]
                        for f in (0.8, 1.1, 1.5, 2.0, 2.8, 4.0):
                            a = z.copy()
                            a[pos[16 * (groups - 1) + 3]] = int(0.52 * one) + 1
                            a[pos[16 * (groups // 2) + int(rng.integers(0, 16))]] = -int(f * one)
                            unit("lone%d" % int(f * one), a, qp)
    return out


def write_case_file(path, hp, units, contexts):
    """the units (job, table, coefficients) and the context-state vectors (log2, comp, 152 states) as the stand-alone checker reads them: int32 magic, count, then per unit
    hop_rdoq_job | hop_estbits | N x N int32; int32 count, then per vector int32 log2, int32 comp, 152 bytes"""
    with open(path, "wb") as f:
        f.write(np.array([FILE_MAGIC, len(units)], np.int32).tobytes())
        for c in units:
            f.write(rdoq_job(hp, c).tobytes()); f.write(np.ascontiguousarray(c["eb"], np.int32).tobytes()); f.write(np.ascontiguousarray(c["src"], np.int32).tobytes())
        f.write(np.array([len(contexts)], np.int32).tobytes())
        for log2, comp, st in contexts:
            f.write(np.array([log2, comp], np.int32).tobytes()); f.write(np.ascontiguousarray(st, np.uint8).tobytes())


def context_vectors(hp, per_size=40):
    """context states for the bit-estimate table: for every (log2 size, component) random state vectors (7-bit state << 1 | MPS: every value below 128 is a state)"""
    rng = np.random.default_rng(7)
    out = []
    for log2 in (2, 3, 4, 5):
        for comp in (0, 1, 2):
            if comp and log2 == 5: continue
            for _ in range(per_size):
                out.append((log2, comp, rng.integers(0, 128, hp.CABAC_CTX_BYTES).astype(np.uint8)))
    return out
