"""GPU: hop_ctx_set_quant_mode -- the leaf step with RDOQ off, as the reference codes with --RDOQ=0 / --RDOQTS=0.

Leaf: hop_tu_rd under {0, 0} gives, for units of every size and kind, the levels of hop_tu_roundtrip (the library's older plain quantiser, sign hiding on one thread)
and of the oracle's restatement of xQuant's plain branch (hop_o_tu_roundtrip_sbh from the samples -- forward transform, then hop_o_quant_flat_sbh: hop_tu_rd hands out
no coefficients; a disagreement of the transform alone would show as hop_tu_roundtrip, whose transform is the leaf's, agreeing where the oracle does not), and the bits hop_coeff_bits counts for those levels -- in the one-kernel form and in the staged pipeline.
Three forms: every class of candidate of tests/test_gpu_walk_codegen.py through the walks side by side, one after the other and the batch steps, under {0, 0} and the
mixed {1, 0}: the same bytes, and other bytes than the default mode's.  Streams: the pictures of tests/golden/stream_rdoq0.npz coded on the device with their mode are the
unmodified reference encoder's .bin byte for byte -- alone, twice in a stack, under per-picture QPs and in the exact wavefront.

Time on one MI355X: the three-forms cases reuse test_gpu_walk_codegen's memo (a run is some 40 ms); the 448x192 picture is coded three times."""
import ctypes
import os

import numpy as np
import pytest

import quant_mode_util as Q
import slicedata_util as U
import stream_util as S
import test_gpu_walk_codegen as WC
from hoputil import oracle, p16
from test_gpu_stream import code_and_filter, stream_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(U.ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


# ---- the leaf ----
W = H = 256
# (component, log2, flags kind): every transform size of luma and chroma, the 4x4 luma DST, transform skip (4x4 only) for luma and chroma
KINDS = [(0, 5, ""), (0, 4, ""), (0, 3, ""), (0, 2, "dst"), (0, 2, ""), (1, 4, ""), (2, 3, ""), (1, 2, ""), (2, 2, ""), (0, 2, "ts"), (1, 2, "ts"), (2, 2, "ts"), (0, 2, "ts-dst")]


def leaf_case(hp, bd):
    """jobs over a 256x256 picture: each kind of unit four times -- intra and inter (no cbf-zero decision: HOP_TU_RD_KEEP), the three scans for the small intra units,
    one without sign hiding; prediction = original + noise with outliers, so that groups hold several levels"""
    rng = np.random.default_rng(7 + bd)
    top = (1 << bd) - 1
    org = [rng.integers(0, top + 1, (H >> (k > 0), W >> (k > 0))).astype(np.int16) for k in range(3)]
    amp = 6 << (bd - 8)
    prd = [np.clip(o + rng.integers(-amp, amp + 1, o.shape) + (rng.random(o.shape) < 0.15) * rng.integers(-20 * amp, 20 * amp + 1, o.shape), 0, top).astype(np.int16) for o in org]
    L = hp.load(); L.hop_cabac_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    rows = []
    cursor = {0: [0, 0], 1: [0, 0], 2: [0, 0]}                              # per component: the next free 32-sample cell (luma) / 16-sample cell (chroma) of its plane
    for comp, log2, kind in KINDS:
        for rep in range(4):
            cx, cy = cursor[comp]
            cell = 32 if comp == 0 else 16
            x, y = cx * cell, cy * cell
            cursor[comp] = [cx + 1, cy] if (cx + 1) * cell < (W if comp == 0 else W // 2) else [0, cy + 1]
            intra = rep < 3                                                 # (the inter leaf knows no DST and no scan but the diagonal)
            rows.append(dict(x=x if comp == 0 else 2 * x, y=y if comp == 0 else 2 * y, comp=comp, log2=log2, ts="ts" in kind, dst=int("dst" in kind and comp == 0 and intra),
                             intra=int(intra), scan=rep if (intra and log2 <= 3) else 0, hide=int(rep != 2 or log2 == 5), qp=int(rng.integers(20, 38)) + 6 * (bd - 8)))
    n = len(rows)
    jobs = np.zeros(n, hp.TU_RD_JOB_DTYPE); snaps = np.zeros((n, hp.CABAC_CTX_BYTES), np.uint8)
    for i, r in enumerate(rows):
        j = jobs[i]
        lam = 0.57 * 2.0 ** ((r["qp"] - 6 * (bd - 8) - 12) / 3.0)
        j["x"], j["y"], j["comp"], j["log2_size"], j["qp_scaled"], j["tr_depth"], j["ctx_index"] = r["x"], r["y"], r["comp"], r["log2"], r["qp"], i % 3, i
        j["sign_hide"], j["use_ts"], j["bit_depth"], j["is_intra"], j["scan_idx"], j["use_dst"] = r["hide"], 1, bd, r["intra"], r["scan"], r["dst"]
        j["flags"] = (hp.HOP_TU_RD_TS if r["ts"] else 0) | (0 if r["intra"] else hp.HOP_TU_RD_KEEP)
        j["lambda_rdoq"], j["lambda_rd"], j["dist_weight"] = lam, lam, (1.0 if r["comp"] == 0 else 1.26)
        assert L.hop_cabac_init(snaps[i].ctypes.data, 2 + i % 2, min(51, r["qp"])) == 0      # (the carried fraction stays 0: bits = counted bits >> 15)
    return org, prd, rows, jobs, snaps


def leaf_run(hp, bd, case, mode, staged=False):
    """hop_tu_rd over the case in a fresh context: (results, levels).  mode: None = the setter is never called, "null" = set then NULL, else (rdoq, rdoq_ts, i_slice)"""
    org, prd, rows, jobs, snaps = case
    old = os.environ.get("HOP_FUSED_LEAF")
    if staged: os.environ["HOP_FUSED_LEAF"] = "0"                             # (read when a context is created: every batch takes the staged pipeline)
    try:
        ctx = hp.Context(W, H, bit_depth=bd)
    finally:
        if staged:
            if old is None: del os.environ["HOP_FUSED_LEAF"]
            else: os.environ["HOP_FUSED_LEAF"] = old
    try:
        ctx.upload_orig(*org)
        for k in range(3):
            ctx.plane_upload("pred", k, prd[k]); ctx.plane_upload("recon", k, np.zeros(org[k].shape, np.int16))
        if mode == "null":
            ctx.set_quant_mode(0, 0, 1); ctx.set_quant_mode(None)
        elif mode is not None:
            ctx.set_quant_mode(*mode)
        res, lv = ctx.tu_rd(jobs, snaps)
        rt = None
        if mode not in (None, "null"):
            tj = [hp.TuJob(r["x"], r["y"], r["comp"], r["log2"], r["dst"], int(r["ts"]), r["qp"], mode[2], r["hide"], r["scan"]) for r in rows]
            rt = ctx.tu_roundtrip(tj)
            cb = np.zeros(len(rows), hp.COEFF_BITS_JOB_DTYPE); off = 0
            for i, r in enumerate(rows):
                chroma = int(r["comp"] != 0); td = i % 3
                cb[i] = (r["log2"], r["comp"], r["scan"], r["hide"], 1, int(r["ts"]), i, 1 + 4 * chroma + (td if chroma else int(td == 0)), off)
                off += 1 << (2 * r["log2"])
            rt = rt + (ctx.coeff_bits(cb, snaps, lv, want_ctx=False)[0],)
        return res, lv, rt
    finally:
        ctx.close()


@pytest.mark.parametrize("i_slice", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_leaf_without_rdoq_is_the_plain_quantiser(hp, bd, i_slice):
    O = oracle(); O.hop_o_tu_roundtrip_sbh.restype = ctypes.c_uint32
    case = leaf_case(hp, bd)
    org, prd, rows, jobs, snaps = case
    res, lv, (rt_res, rt_lv, bits) = leaf_run(hp, bd, case, (0, 0, i_slice))
    on = leaf_run(hp, bd, case, None)
    off = hidden = 0
    for i, r in enumerate(rows):
        N = 1 << r["log2"]; s = 1 if r["comp"] else 0
        x, y = r["x"] >> s, r["y"] >> s
        mine = lv[off:off + N * N]
        assert np.array_equal(mine, rt_lv[off:off + N * N]) and int(res[i]["abs_sum"]) == rt_res[i][0], ("hop_tu_roundtrip", i, r)
        o = np.ascontiguousarray(org[r["comp"]][y:y + N, x:x + N]); p = np.ascontiguousarray(prd[r["comp"]][y:y + N, x:x + N])
        want = np.zeros(N * N, np.int32); rec = np.zeros(N * N, np.int16); sse = ctypes.c_uint32(0)
        wsum = O.hop_o_tu_roundtrip_sbh(bd, r["qp"], i_slice, r["dst"], int(r["ts"]), N, r["hide"], r["scan"], p16(o), p16(p), want.ctypes.data_as(ctypes.c_void_p), p16(rec), ctypes.byref(sse))
        assert np.array_equal(mine, want) and int(res[i]["abs_sum"]) == wsum, ("oracle", i, r)
        assert int(res[i]["bits"]) == int(bits[i]) >> 15, ("hop_coeff_bits", i, r, int(res[i]["bits"]), int(bits[i]))
        if r["hide"]:
            plain = np.zeros(N * N, np.int32)
            O.hop_o_tu_roundtrip_sbh(bd, r["qp"], i_slice, r["dst"], int(r["ts"]), N, 0, 0, p16(o), p16(p), plain.ctypes.data_as(ctypes.c_void_p), p16(rec), ctypes.byref(sse))
            hidden += int(not np.array_equal(plain, want))
        off += N * N
    assert hidden > len(rows) // 4 and not np.array_equal(lv, on[1])        # the case is what it says: sign hiding acts, and RDOQ gives other levels
    # the staged pipeline (k_turd_setup_mode, k_quant_flat): the same bytes
    st = leaf_run(hp, bd, case, (0, 0, i_slice), staged=True)
    assert st[0].tobytes() == res.tobytes() and np.array_equal(st[1], lv)


def test_leaf_mixed_modes_and_the_default(hp):
    """{1, 0} and {0, 1}: a unit follows the switch of its own kind, in both forms of the leaf; {1, 1} set explicitly, and NULL after another mode, give the bytes of a
    context that never called the setter"""
    case = leaf_case(hp, 8)
    rows = case[2]
    never = leaf_run(hp, 8, case, None)
    flat = leaf_run(hp, 8, case, (0, 0, 0))
    for mode in ((1, 0, 0), (0, 1, 0)):
        got = leaf_run(hp, 8, case, mode); staged = leaf_run(hp, 8, case, mode, staged=True)
        assert staged[0].tobytes() == got[0].tobytes() and np.array_equal(staged[1], got[1]), mode
        off = 0
        for i, r in enumerate(rows):
            n2 = 1 << (2 * r["log2"])
            src = flat if (mode[1] if r["ts"] else mode[0]) == 0 else never
            assert np.array_equal(got[1][off:off + n2], src[1][off:off + n2]) and got[0][i].tobytes() == src[0][i].tobytes(), (mode, i, r)
            off += n2
    for mode in ((1, 1, 0), (1, 1, 1), "null"):
        got = leaf_run(hp, 8, case, mode)
        assert got[0].tobytes() == never[0].tobytes() and np.array_equal(got[1], never[1]), mode
    staged = leaf_run(hp, 8, case, None, staged=True)
    assert staged[0].tobytes() == never[0].tobytes() and np.array_equal(staged[1], never[1])


# ---- the three forms of the chain ----
class ModeClass(tuple):
    """a class of tests/test_gpu_walk_codegen.py with a quantiser mode: that file memoises its runs by class, so the mode has to be part of the key"""
    def __new__(cls, base, mode):
        self = super().__new__(cls, base); self.mode = mode
        return self

    def __eq__(self, other): return tuple(self) == tuple(other) and getattr(other, "mode", None) == self.mode
    def __ne__(self, other): return not self == other
    def __hash__(self): return hash((tuple(self), self.mode))


class ModeBinding:
    """the binding with contexts that set a quantiser mode as they are made (test_gpu_walk_codegen._run makes its own)"""
    def __init__(self, hp, mode): self._hp, self._mode = hp, mode
    def __getattr__(self, name): return getattr(self._hp, name)

    def Context(self, *a, **kw):
        ctx = self._hp.Context(*a, **kw)
        ctx.set_quant_mode(*self._mode)
        return ctx


@pytest.mark.parametrize("content", ["noisy", "flat"])
@pytest.mark.parametrize("cls", WC.CLASSES, ids=WC._ident)
def test_three_forms_agree_without_rdoq(hp, cls, content):
    n = 5
    default = WC._run(hp, cls, n, content, WC.FORMS[0][1])
    for mode in ((0, 0, 0), (1, 0, 0)):
        mc, mhp = ModeClass(cls, mode), ModeBinding(hp, mode)
        ref = WC._run(mhp, mc, n, content, WC.FORMS[2][1])
        for form, env in WC.FORMS[:2]:
            got = WC._run(mhp, mc, n, content, env)
            for name in ref:
                assert got[name] == ref[name], (WC._ident(cls), mode, content, form, "differs from the batch steps in", name)
        if content == "noisy" and mode == (0, 0, 0):
            assert ref["d_coef"] != default["d_coef"], (WC._ident(cls), "RDOQ off codes the default mode's levels")
        if content == "flat":
            assert not np.frombuffer(ref["d_coef"], np.int32).any()


# ---- streams ----
def coded_stream(hp, key, mode, exact=False, wrong_i_slice=True):
    """the case through hop_encode_frame, hop_deblock_frame, hop_sao_frame, hop_access_unit_write(hash = 1) under the mode; i_slice is set to what the slice is NOT:
    hop_encode_frame takes it from plain_intra"""
    c = Q.CASES[key]
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], slots=0 if c["plain"] else 16)
    try:
        ctx.set_quant_mode(mode[0], mode[1], (0 if c["plain"] else 1) if wrong_i_slice else (1 if c["plain"] else 0))
        if exact: ctx.set_exact(1)
        parts, sao = code_and_filter(ctx, c, c["pictures"][0])
        return ctx.access_unit_write(parts, None, sao, poc=0, parameter_sets=1, hash=1, guard=256, **stream_args(c))[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("key,mode", Q.STREAMS, ids=Q.IDS)
def test_device_stream_equals_the_reference_encoder_without_rdoq(hp, key, mode):
    want = Q.stream(key, mode)
    got = coded_stream(hp, key, mode)
    assert got == want, "%s %s: %s" % (key, mode, S.first_difference(got, want))
    assert got != Q.stream(key, (1, 1))


def test_exact_wavefront_codes_the_same_stream(hp):
    key, mode = "448x192_seed3_mi15_wpp", (0, 0)
    want = Q.stream(key, mode)
    got = coded_stream(hp, key, mode, exact=True, wrong_i_slice=False)
    assert got == want, S.first_difference(got, want)


def test_stack_of_two_with_and_without_picture_qps(hp):
    key = "64x64_raster"
    c = Q.CASES[key]
    want = Q.stream(key, (0, 0))
    Y, Cb, Cr = c["pictures"][0]
    ctx = hp.Context(64, 64, pictures=2, slots=16)
    try:
        ctx.upload_orig(ctx.stack([Y, Y]), ctx.stack([Cb, Cb], True), ctx.stack([Cr, Cr], True))
        ctx.set_quant_mode(0, 0, 0)
        for qps in (None, [32, 32]):
            ctx.set_picture_qps(qps)
            parts = ctx.encode_frame(32, 16, 0, None, wpp=0, wavefront_lag=5)[3]
            ctx.deblock_frame(parts, 32)
            frac = ctx.rd_fraction_download()
            sao = ctx.sao_frame_pictures([(U.sao_lambdas(32), 3, 32, int(frac[k])) for k in range(2)])
            data, sizes = ctx.access_unit_write(parts, None, sao, poc=0, parameter_sets=1, hash=1, guard=256, **stream_args(c))
            assert len(sizes) == 2 and int(sizes.sum()) == len(data)
            for k in range(2):
                au = data[int(sizes[:k].sum()):int(sizes[:k + 1].sum())]
                assert au == want, "picture QPs %s, picture %d: %s" % (qps, k, S.first_difference(au, want))
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable(hp):
    case = leaf_case(hp, 8)
    org, prd, rows, jobs, snaps = case
    ctx = hp.Context(W, H)
    try:
        ctx.upload_orig(*org)
        for k in range(3):
            ctx.plane_upload("pred", k, prd[k]); ctx.plane_upload("recon", k, np.zeros(org[k].shape, np.int16))
        ctx.set_quant_mode(0, 0, 0)
        flat = ctx.tu_rd(jobs, snaps)
        for bad in ((2, 1, 0), (1, -1, 0), (0, 7, 1)):
            with pytest.raises(hp.HopError) as e:
                ctx.set_quant_mode(*bad)
            assert e.value.code == -1 and "hop_ctx_set_quant_mode" in str(e.value)
        again = ctx.tu_rd(jobs, snaps)                                       # the mode stayed
        assert again[0].tobytes() == flat[0].tobytes() and np.array_equal(again[1], flat[1])
        # a view cannot set the mode and reads its parent's, also one set after the view was made
        L = ctx.L
        L.hop_ctx_create_view.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; L.hop_ctx_set_quant_mode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.hop_ctx_destroy.argtypes = [ctypes.c_void_p]
        vh = ctypes.c_void_p()
        assert L.hop_ctx_create_view(ctx.h, ctypes.byref(vh)) == 0
        m = hp.QuantMode(1, 1, 0)
        assert L.hop_ctx_set_quant_mode(vh, ctypes.byref(m)) == -1 and L.hop_ctx_set_quant_mode(vh, None) == -1
        assert b"view" in L.hop_last_error(vh)
        res = np.zeros(len(jobs), hp.TU_RD_RESULT_DTYPE); lv = np.zeros(len(flat[1]), np.int32)
        def view_tu_rd():
            assert L.hop_tu_rd(vh, len(jobs), jobs.ctypes.data, len(snaps), snaps.ctypes.data, res.ctypes.data, lv.ctypes.data) == 0
            return res.tobytes(), lv.copy()
        r0, l0 = view_tu_rd()
        assert r0 == flat[0].tobytes() and np.array_equal(l0, flat[1])
        ctx.set_quant_mode(None)
        on = ctx.tu_rd(jobs, snaps)
        r1, l1 = view_tu_rd()
        assert r1 == on[0].tobytes() and np.array_equal(l1, on[1]) and not np.array_equal(l1, l0)
        L.hop_ctx_destroy(vh)
    finally:
        ctx.close()
