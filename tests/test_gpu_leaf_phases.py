"""GPU: the leaf step with its serial stages in phases (csrc/k_leaf_fused.inl: bit-estimate table and RDOQ's position-only work on all lanes, the recurrences on lane 0)
against the staged pipeline, whose k_turd_setup and k_rdoq keep the one-lane bodies (turd_setup_body, rdoq_tu).  tests/test_rdoq_phased_cpu.py compares the two forms of
the same source on the host; here the device runs them.

* hop_tu_rd_device as one kernel (the default) against the staged 13 launches (HOP_FUSED_LEAF=0): batches of 1 and 5 units of each size, a batch of 4x4 and 8x8 units only and
  a mixed one, luma and chroma, inter and intra leaves, with and without sign hiding.  The residual of a unit is the inverse transform of a generated unit of
  tests/rdoq_cases.py (zero, first, last, saturated, dense, sparse, lone), so the coefficients the device's forward transform hands to RDOQ are that family's up to
  rounding.  Levels, hop_tu_rd_result records and the reconstruction planes (intra leaves write them) are compared byte for byte.
* The candidate walks, which run the same leaf bodies -- the 4x4 / 8x8 units of a node a wave each, with rounds in which a wave has no unit --: inter 8x8 / 16x16 / 32x32,
  intra 16x16 and intra 8x8 NxN, 1 and 5 candidates, against the batch steps (HOP_WALK=0); and the classes whose units are 32x32 (work area in HBM) and 16x16 (in LDS), inter
  and intra, with the work buffer pre-filled with 0 and with 255 (HOP_WALK_FILL).  The cases are test_gpu_walk_codegen's (its _case / _run, memoised across both files).

No test here asserts a time.  The file runs in a few seconds: contexts of 128x128 (x 5 pictures for the walks), batches of at most 14 units."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import rdoq_cases
from hoputil import ROOT
from test_gpu_walk_codegen import _env, _ident, _run

pytestmark = pytest.mark.gpu

W, H = 128, 128
_memo = {}


@pytest.fixture(scope="module")
def hp():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _dct(n):
    k = np.arange(n)[:, None]; x = np.arange(n)[None, :]
    m = np.cos(np.pi * (2 * x + 1) * k / (2 * n)) * np.sqrt(2.0 / n); m[0] /= np.sqrt(2.0)
    return m


def _residual(c):
    """the residual block whose forward transform is about the unit's coefficients: the core transform is the orthonormal DCT scaled by 2^(15 - bit depth - log2)"""
    n = 1 << c["log2"]; m = _dct(n)
    r = m.T @ (c["src"].reshape(n, n) / 2.0 ** (7 - c["log2"])) @ m
    return np.clip(np.rint(r), -255, 255).astype(np.int32)


def _batches(hp):
    """{name: (jobs, snapshots, planes)}; the units of a batch tile the 128x128 picture, every unit at its own place in all three planes"""
    if "batches" in _memo: return _memo["batches"]
    L = rdoq_cases.bind(hp.load())
    units = rdoq_cases.unit_cases(L, hp)
    fam = lambda c: c["name"].split()[-1].rstrip("0123456789")
    pick = lambda log2, comp: [c for c in units if c["log2"] == log2 and (c["comp"] != 0) == (comp != 0)]
    rng = np.random.default_rng(5)
    def batch(specs):
        n = len(specs)
        org = [np.full((H >> (k > 0), W >> (k > 0)), 128, np.int16) for k in range(3)]; pred = [a.copy() for a in org]
        jobs = np.zeros(n, hp.TU_RD_JOB_DTYPE); snaps = np.zeros((n, hp.CABAC_CTX_BYTES), np.uint8)
        for t, (c, comp) in enumerate(specs):
            x, y = 32 * (t % 4), 32 * (t // 4)                               # luma position; a chroma unit of up to 16x16 sits at (x / 2, y / 2)
            assert y + 32 <= H
            r = _residual(c); N = r.shape[0]; s = 1 if comp else 0
            p = np.clip(128 - r // 2, 0, 255); o = np.clip(p + r, 0, 255)
            org[comp][y >> s:(y >> s) + N, x >> s:(x >> s) + N] = o; pred[comp][y >> s:(y >> s) + N, x >> s:(x >> s) + N] = p
            j = jobs[t]
            j["x"], j["y"], j["comp"], j["log2_size"], j["qp_scaled"], j["tr_depth"], j["ctx_index"] = x, y, comp, c["log2"], c["qp"], c["tr"], t
            j["sign_hide"], j["use_ts"], j["bit_depth"], j["is_intra"], j["scan_idx"] = c["sh"], 1, 8, c["intra"], c["scan"]
            j["use_dst"] = int(c["intra"] and c["log2"] == 2 and comp == 0)
            j["lambda_rdoq"], j["lambda_rd"], j["dist_weight"] = c["lam"], c["lam"], float(rng.choice([1.0, 1.26]))
            assert L.hop_cabac_init(snaps[t].ctypes.data, int(rng.integers(0, 5)), c["qp"]) == 0
            left = int(rng.integers(0, 32768)); snaps[t, 150], snaps[t, 151] = left & 255, left >> 8
        return jobs, snaps, org, pred
    out = {}
    for log2 in (2, 3, 4, 5):
        cs = pick(log2, 0); by = {}
        for c in cs: by.setdefault(fam(c), []).append(c)
        # one unit (dense, sign hiding on) and five (one of each family with levels; scans and sign_hide as they come)
        dense = [c for c in by["dense"] if c["sh"]][0]
        out["%dx%d n=1" % (1 << log2, 1 << log2)] = batch([(dense, 0)])
        five = [by[f][i % len(by[f])] for i, f in enumerate(("dense", "saturated", "sparse", "last", "lone" if log2 >= 3 else "first"))]
        out["%dx%d n=5" % (1 << log2, 1 << log2)] = batch([(c, 0) for c in five])
    of = lambda log2: [(c, comp) for comp in (0, 1, 2) for c in pick(log2, comp) if fam(c) in ("dense", "zero") and c["sh"]]
    small = [u for pair in zip(of(2), of(3)) for u in pair]           # 4x4 and 8x8 units in turn, every component
    out["all small n=5"] = batch(small[:5])
    out["all small n=14"] = batch(small[:14])
    mixed = []
    for log2, comp in rdoq_cases.SIZES:
        cs = [c for c in pick(log2, comp) if fam(c) in ("dense", "sparse", "lone")]
        mixed += [(cs[0], 2 * (comp != 0)), (cs[len(cs) // 2], comp)]
    out["mixed n=14"] = batch(mixed)
    _memo["batches"] = out
    return out


def _tu_rd(hp, name, staged):
    """one batch through hop_tu_rd_device -> (levels, results, the three reconstruction planes), bytes"""
    key = (name, staged)
    if key in _memo: return _memo[key]
    import torch
    jobs, snaps, org, pred = _batches(hp)[name]
    n = len(jobs); offs = np.concatenate([[0], np.cumsum(1 << (2 * jobs["log2_size"].astype(np.int64)))]).astype(np.int64); tot = int(offs[-1])
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    with _env({}):
        old = os.environ.pop("HOP_FUSED_LEAF", None)
        if staged: os.environ["HOP_FUSED_LEAF"] = "0"
        try:
            ctx = hp.Context(W, H)                                       # (HOP_FUSED_LEAF is read when a context is created)
        finally:
            os.environ.pop("HOP_FUSED_LEAF", None)
            if old is not None: os.environ["HOP_FUSED_LEAF"] = old
        try:
            ctx.upload_orig(*org)
            for k in range(3):
                ctx.plane_upload("pred", k, pred[k]); ctx.plane_upload("recon", k, np.full_like(pred[k], 77))
            d_jobs, d_snap, d_off = up(jobs), up(snaps), up(offs[:-1])
            d_lv = torch.full((tot * 4,), 0x5A, dtype=torch.uint8, device=dev); d_res = torch.zeros(n * hp.TU_RD_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            fn = ctx.L.hop_tu_rd_device; fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
            ctx._chk(fn(ctx.h, n, d_jobs.data_ptr(), d_snap.data_ptr(), d_off.data_ptr(), tot, d_lv.data_ptr(), d_res.data_ptr()), "hop_tu_rd_device")
            ctx.sync()
            got = dict(levels=d_lv.cpu().numpy().tobytes(), results=d_res.cpu().numpy().tobytes())
            for k in range(3): got["recon%d" % k] = ctx.recon_download(k).tobytes()
        finally:
            ctx.close()
    _memo[key] = got
    return got


BATCHES = ["%dx%d n=%d" % (s, s, n) for s in (4, 8, 16, 32) for n in (1, 5)] + ["all small n=5", "all small n=14", "mixed n=14"]


@pytest.mark.parametrize("name", BATCHES)
def test_fused_leaf_gives_the_staged_pipeline_byte_for_byte(hp, name):
    ref = _tu_rd(hp, name, True); got = _tu_rd(hp, name, False)
    for what in ref:
        assert got[what] == ref[what], (name, "the one-kernel leaf differs from the staged pipeline in", what)
    res = np.frombuffer(ref["results"], hp.TU_RD_RESULT_DTYPE)
    assert (res["cost"] > 0).any()


def test_the_batches_hold_what_they_say(hp):
    """every size in the mixed batch, both components classes, inter and intra leaves, sign hiding on and off somewhere; levels come out"""
    B = _batches(hp)
    jobs = np.concatenate([b[0] for b in B.values()])
    assert set(jobs["log2_size"]) == {2, 3, 4, 5} and set(jobs["comp"]) == {0, 1, 2} and set(jobs["is_intra"]) == {0, 1} and set(jobs["sign_hide"]) == {0, 1}
    assert set(B["mixed n=14"][0]["log2_size"]) == {2, 3, 4, 5} and set(B["all small n=5"][0]["log2_size"]) <= {2, 3}
    for name in ("4x4 n=5", "8x8 n=5", "16x16 n=5", "32x32 n=5"):        # (each holds a saturated unit)
        assert np.frombuffer(_tu_rd(hp, name, True)["levels"], np.int32).any(), name


WALK_CLASSES = [("inter", 3, 0), ("inter", 4, 0), ("inter", 5, 0), ("intra", 4, 0), ("intra", 3, 1)]
FILL_CLASSES = [("inter", 5, 0), ("intra", 5, 0)]                         # 32x32 luma units (work area in HBM) over 16x16 chroma units (in LDS)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cls", WALK_CLASSES, ids=_ident)
def test_walks_give_the_batch_steps_byte_for_byte(hp, cls, n):
    ref = _run(hp, cls, n, "noisy", {"HOP_WALK": "0"}); got = _run(hp, cls, n, "noisy", {})
    for name in ref:
        assert got[name] == ref[name], (_ident(cls), n, "the walk differs from the batch steps in", name)
    assert np.frombuffer(ref["d_coef"], np.int32).any()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cls", FILL_CLASSES, ids=_ident)
def test_walks_do_not_read_what_the_work_area_held(hp, cls, n):
    ref = _run(hp, cls, n, "noisy", {})
    for fill in (0, 255):
        got = _run(hp, cls, n, "noisy", {}, fill)
        for name in ref:
            assert got[name] == ref[name], (_ident(cls), n, "HOP_WALK_FILL=%d" % fill, "changes", name)
