"""GPU: the stage stamps of the candidate walks (csrc/k_walk_stamps.inl; hop_walk_stamps_* of include/hophip.h) in the diagnostic build libhophip_stamps.so.

What is pinned here is the INSTRUMENT, not what it measures: no test asserts a share or a time.
  1. the product library refuses the stamps' entries and says which library has them;
  2. the stamps change no result: the stamps build against the product build through tests/test_gpu_walk_codegen.py's _run, every output and the three planes, for the
     smallest classes that reach every stamped body (wave leaves at 8x8, whole-workgroup leaves at 16 / 32, bands and chroma on the intra side);
  3. the accounting closes: per kernel the stages add up to the span between the workgroup's first and last stamp EXACTLY (two independent measurements: a segment left
     open, counted twice or not flushed breaks it), the serial stages of a leaf are visited equally often, rows of classes that did not run stay zero, reset zeroes;
     the same, with the bytes, for k_intra_walk (HOP_WALK_CAND=0), which the default form never launches;
  4. the units: a workgroup's span on the 100 MHz counter is not longer than its kernel between two HIP events.
Both libraries live in this process, each behind a fresh instance of the hophip module; HOP_LIB is set only while the stamps instance loads and runs.
Time: some 30 small runs on top of those test_gpu_walk_codegen.py has memoised, a few seconds in all."""
import contextlib
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_walk_codegen as wc
from hoputil import ROOT

pytestmark = pytest.mark.gpu

STAMPS = os.path.join(ROOT, "hevc-hop_amd", "libhophip_stamps.so")
# (side, log2 of the CU, NxN)
CLASSES = [("inter", 3, 0), ("inter", 4, 0), ("inter", 5, 0), ("intra", 4, 0), ("intra", 3, 1)]
LEAF_KERNELS = ("k_inter_walk", "k_iw_cand", "k_iw_chroma")            # every workgroup of these codes at least one transform unit


def _fresh():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@contextlib.contextmanager
def _lib(path):
    """HOP_LIB = path (None: unset, the product library) while the block runs"""
    old = os.environ.get("HOP_LIB")
    try:
        os.environ.pop("HOP_LIB", None)
        if path: os.environ["HOP_LIB"] = path
        yield
    finally:
        os.environ.pop("HOP_LIB", None)
        if old is not None: os.environ["HOP_LIB"] = old


@pytest.fixture(scope="module")
def product():
    with _lib(None):
        m = _fresh(); m.load()
    assert m.LIB_PATH.endswith("libhophip.so")
    return m


@pytest.fixture(scope="module")
def stamps():
    with _lib(STAMPS):
        m = _fresh(); m.load()
    assert m.LIB_PATH == STAMPS
    return m


def _run_product(product, cls, n, content):
    with _lib(None):
        return wc._run(product, cls, n, content, {})


def _run_stamps(stamps, cls, n, content, again=False):
    """the same case through the stamps library (the library's path is part of the memo's key); again: run it even if the memo holds it"""
    env = {"HOP_LIB": STAMPS}
    if again: wc._runs.pop((cls, n, content, tuple(sorted(env.items())), None), None)
    with _lib(STAMPS):
        return wc._run(stamps, cls, n, content, env)


def test_product_library_refuses_and_names_the_stamps_library(product):
    with _lib(None):
        ctx = product.Context(64, 64)
        try:
            for call in (lambda: ctx.walk_stamps(product.HOP_WSK_INTER_WALK, 4), ctx.walk_stamps_reset, ctx.walk_stamps_probe):
                with pytest.raises(product.HopError, match="libhophip_stamps.so") as e:
                    call()
                assert e.value.code == product.HOP_ERR_STATE and "HOP_LIB" in str(e.value)
        finally:
            ctx.close()


@pytest.mark.parametrize("content", ["noisy", "flat"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cls", CLASSES, ids=wc._ident)
def test_stamps_build_gives_the_product_builds_bytes(product, stamps, cls, n, content):
    ref = _run_product(product, cls, n, content)
    got = _run_stamps(stamps, cls, n, content)
    assert set(got) == set(ref) and {"recon0", "recon1", "recon2", "d_cost", "d_coef"} <= set(ref)
    for name in ref:
        assert got[name] == ref[name], (wc._ident(cls), n, content, "the stamps build differs from the product in", name)


def _rows(stamps, ctx):
    """every row of the table: {(kernel name, log2_cu, nxn): (cycles, visits, total)}"""
    return {(kn, lg, nxn): ctx.walk_stamps(k, lg, nxn) for k, kn in enumerate(stamps.HOP_WSK_NAMES) for lg in (3, 4, 5, 6) for nxn in (0, 1)}


def _is_zero(row):
    cyc, vis, tot = row
    return not cyc.any() and not vis.any() and not any(tot.values())


@pytest.mark.parametrize("cls", CLASSES, ids=wc._ident)
def test_stages_add_up_to_the_workgroups_span(stamps, cls):
    S = stamps
    side, lg, nxn = cls
    n = 5
    with _lib(STAMPS):
        ctx = S.Context(64, 64)
    try:
        ctx.walk_stamps_reset()
        assert all(_is_zero(r) for r in _rows(S, ctx).values())
        _run_stamps(S, cls, n, "noisy", again=True)
        rows = _rows(S, ctx)
        ran = {key: r for key, r in rows.items() if not _is_zero(r)}
        # only this class's rows, and of its side's kernels
        want = {"k_inter_walk"} if side == "inter" else {"k_iw_begin", "k_iw_cand", "k_iw_pick", "k_iw_chroma", "k_iw_finish"}
        assert {key[1:] for key in ran} == {(lg, nxn)} and {key[0] for key in ran} == want, sorted(ran)
        wg = {key[0]: r[2]["workgroups"] for key, r in ran.items()}
        npu = 4 if nxn else 1
        if side == "inter": assert wg == {"k_inter_walk": n}
        else:                                                          # the grids of hop_launch_intra_walk; a pass a CU's list does not have leaves no row
            assert wg["k_iw_begin"] == n and wg["k_iw_pick"] == n * npu and wg["k_iw_chroma"] == 5 * n and wg["k_iw_finish"] == n
            assert n * npu <= wg["k_iw_cand"] <= n * npu * 10
        visited = np.zeros(S.HOP_WS_COUNT, np.uint64)
        for (kn, _, _), (cyc, vis, tot) in ran.items():
            print(kn, wc._ident(cls), "cycles", cyc.tolist(), "visits", vis.tolist(), tot)
            assert int(cyc.sum()) == tot["cycles"] > 0, (kn, "stages", int(cyc.sum()), "span", tot["cycles"])
            assert 0 < tot["max_realtime_ticks"] <= tot["realtime_ticks"] <= tot["workgroups"] * tot["max_realtime_ticks"], (kn, tot)
            assert vis[S.HOP_WS_LEAF_ESTBITS] == vis[S.HOP_WS_LEAF_RDOQ] == vis[S.HOP_WS_LEAF_BITS] == vis[S.HOP_WS_LEAF_DECIDE], (kn, vis.tolist())
            if kn in LEAF_KERNELS: assert vis[S.HOP_WS_LEAF_ESTBITS] > 0 and cyc[S.HOP_WS_LEAF_RDOQ] > 0, (kn, vis.tolist())
            assert not cyc[vis == 0].any(), (kn, "cycles in a stage never opened")
            visited += vis
        for st in (S.HOP_WS_NODE_SINGLE, S.HOP_WS_CU_BITS, S.HOP_WS_TAIL):
            assert visited[st] > 0, ("never visited", S.walk_stamps_stage_names(ctx.L)[st])
        ctx.walk_stamps_reset()
        assert all(_is_zero(r) for r in _rows(S, ctx).values())
    finally:
        ctx.close()


@pytest.mark.parametrize("cls", [("intra", 4, 0), ("intra", 3, 1)], ids=wc._ident)
def test_one_after_the_other_form_is_stamped_too(product, stamps, cls):
    """HOP_WALK_CAND=0 sends an intra class through k_intra_walk, the seventh stamped kernel: the product's bytes, one row, one workgroup per CU, and the stages add up"""
    S = stamps
    n, env = 5, {"HOP_LIB": STAMPS, "HOP_WALK_CAND": "0"}
    with _lib(None):
        ref = wc._run(product, cls, n, "noisy", {"HOP_WALK_CAND": "0"})
    with _lib(STAMPS):
        ctx = S.Context(64, 64)
    try:
        ctx.walk_stamps_reset()
        wc._runs.pop((cls, n, "noisy", tuple(sorted(env.items())), None), None)
        with _lib(STAMPS):
            got = wc._run(S, cls, n, "noisy", env)
        for name in ref:
            assert got[name] == ref[name], (wc._ident(cls), "the stamps build differs from the product in", name)
        ran = {key: r for key, r in _rows(S, ctx).items() if not _is_zero(r)}
        assert set(ran) == {("k_intra_walk", cls[1], cls[2])}, sorted(ran)
        cyc, vis, tot = ran[("k_intra_walk", cls[1], cls[2])]
        print("k_intra_walk", wc._ident(cls), "cycles", cyc.tolist(), "visits", vis.tolist(), tot)
        assert tot["workgroups"] == n and int(cyc.sum()) == tot["cycles"] > 0
        assert vis[S.HOP_WS_LEAF_ESTBITS] == vis[S.HOP_WS_LEAF_RDOQ] == vis[S.HOP_WS_LEAF_BITS] == vis[S.HOP_WS_LEAF_DECIDE] > 0
        assert vis[S.HOP_WS_NODE_SINGLE] > 0 and vis[S.HOP_WS_CU_BITS] > 0 and vis[S.HOP_WS_TAIL] > 0 and not cyc[vis == 0].any()
    finally:
        ctx.close()


def test_a_workgroup_does_not_outlast_its_kernel(stamps):
    """n = 1, inter 16x16: the one workgroup's span in 10 ns ticks against the kernel's HIP-event time (hop_profile_read).  No margin: the events enclose the kernel."""
    S = stamps
    cls = ("inter", 4, 0)
    seen = []

    class Profiled(S.Context):                                         # the context _run makes, with the events on and read before it goes
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.profile(on=True, reset=True)

        def close(self):
            if self.h: seen.append(self.profile(read=S.HOP_K_WALK_INTER + 1))
            super().close()

    with _lib(STAMPS):
        ctl = S.Context(64, 64)
    plain = S.Context
    try:
        ctl.walk_stamps_reset()
        S.Context = Profiled
        _run_stamps(S, cls, 1, "noisy", again=True)
    finally:
        S.Context = plain
    try:
        _, _, tot = ctl.walk_stamps(S.HOP_WSK_INTER_WALK, 4, 0)
    finally:
        ctl.close()
    timed = [p for p in seen if p[0]]
    assert len(timed) == 1 and timed[0][0] == 1 and timed[0][2] == 1, seen      # one launch of one candidate
    ms = timed[0][1]
    print("workgroup %.3f us on the 100 MHz counter, kernel %.3f us between its events" % (tot["max_realtime_ticks"] * 0.01, ms * 1000))
    assert tot["workgroups"] == 1 and tot["max_realtime_ticks"] == tot["realtime_ticks"] > 0
    assert tot["max_realtime_ticks"] * 1e-5 <= ms, (tot, ms)
