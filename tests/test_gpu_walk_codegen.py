"""GPU: the candidate walks (csrc/k_walk.inl) against the staged chains, and against what their work buffers held.

The walk kernels run the batch steps' own bodies; how the compiler lays those bodies out (what is a function of its own, what stays in registers, which address space a
pointer is known to have) must change no byte of any result.  Every class of candidate the RD spine sends through hop_inter_cu_device_classes / hop_intra_cu_device_classes
runs here in the three forms of the chain -- the walks with a PU's candidate passes side by side (the default), one after the other (HOP_WALK_CAND=0), and the batch steps
(HOP_WALK=0) -- and every output, for intra also the context's three reconstruction planes, must be the same bytes.  HOP_WALK_FILL=<byte> fills the walks' work buffer before
the launch: a walk reads no word of it that it has not written, so the byte must not show in any output either.

One 128x128 picture per candidate (a stacked context of five), the CU at (64, 64) so that a 64x64 CU has neighbours too; n = 1 and n = 5 candidates per class (the grids and
the lane-or-block choice of the coder bodies treat a single candidate differently); noisy content (levels of every kind: sign hiding, zeroed coefficient groups, moved last
positions, transform skip) and a flat picture (every level zero).

What this file does not see: the batch steps share the device bodies with the walks (leaf_serial, the hopd_lds bodies), so a miscompile common to all three forms would
pass here; the replays of the reference encoder's recorded calls in tests/test_gpu_tq_intra.py and the goldens of tests/test_gpu_spine.py pin the bodies themselves.
Time: 60 cases over some 150 small runs (a context each, memoised across the tests), 5.3 s in all on one MI355X, the slowest case (intra 64x64, noisy) 0.42 s; the
budget for the file is 20 s."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from hoputil import ROOT

pytestmark = pytest.mark.gpu

PICS, W, H, X0, Y0 = 5, 128, 128, 64, 64
FORMS = [("side by side", {}), ("one after the other", {"HOP_WALK_CAND": "0"}), ("batch steps", {"HOP_WALK": "0"})]
INTER_OUT = ("d_results", "d_coef", "d_ctx_after", "d_finals", "d_bits", "d_skipped", "d_cost", "d_ctx_out", "d_cu_ctx_out")
INTRA_OUT = ("d_sresults", "d_results", "d_cresults", "d_coef", "d_reco_y", "d_reco_c", "d_syntax_out", "d_dist", "d_bits", "d_cost", "d_ctx_out", "d_cu_ctx_out")
# (side, log2 of the CU, NxN)
CLASSES = [("inter", 3, 0), ("inter", 4, 0), ("inter", 5, 0), ("inter", 6, 0), ("intra", 3, 0), ("intra", 4, 0), ("intra", 5, 0), ("intra", 6, 0), ("intra", 3, 1)]
FILL_CLASSES = [("inter", 4, 0), ("inter", 6, 0), ("intra", 4, 0), ("intra", 6, 0), ("intra", 3, 1)]      # (8x8 NxN exists for intra only)
_ENV = ("HOP_WALK", "HOP_WALK_CAND", "HOP_WALK_FILL")
_runs = {}                                                             # every (class, n, content, form, fill) runs once per session


@pytest.fixture(scope="module")
def hp():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@contextlib.contextmanager
def _env(settings):
    old = {k: os.environ.get(k) for k in _ENV}
    try:
        for k in _ENV: os.environ.pop(k, None)
        os.environ.update(settings)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None: os.environ[k] = v


def _units(lg, bx, by, N, part, edge=True):
    """availability of the neighbouring 4-sample units of the N x N block at (bx, by) of a CU of size 1 << lg at (X0, Y0), first unit `part` in z order, as an encoder
    hands it over (tests/test_gpu_intra_final_pass.py:causal_avail): below-left (bottom-most first) and left upwards, the corner, above, above-right; a unit is available if
    it lies above the CU or beside it, or inside the CU before the block in coding order -- AND inside the picture: the CU reaches the picture's right and bottom edge, and
    a unit called available out there is read through the row pitch in the picture and not copied into a candidate's band (the forms would then read different samples).
    edge=False leaves that rule out: then this is causal_avail's rule exactly, which _causal_avail asserts wherever causal_avail is defined, so the two cannot drift"""
    from test_gpu_intra_final_pass import _zidx
    cu = 1 << lg; U = N // 4
    def ok(sx, sy):
        if edge and (X0 + sx >= W or Y0 + sy >= H): return False
        if sy < 0: return True
        if sx < 0: return sy < cu
        return sx < cu and sy < cu and _zidx(sx // 4, sy // 4) < part
    units = [(bx - 1, by + 4 * (2 * U - 1 - u)) for u in range(2 * U)] + [(bx - 1, by - 1)] + [(bx + 4 * j, by - 1) for j in range(2 * U)]
    return [int(ok(sx, sy)) for sx, sy in units]


def _causal_avail(lg):
    """hop_intra_rqt_opt.avail: per node of the transform tree that can be predicted (4x4 .. 32x32; the root of a 64x64 CU is no transform unit and has no entry) one bit
    per unit of _units"""
    from test_gpu_intra_final_pass import _zx, _zy, causal_avail
    first = (0, 1, 5, 21, 85)
    def table(edge):
        out = np.zeros(341, np.uint64)
        for d in range(lg - 1):
            log2 = lg - d
            if log2 > 5: continue
            for idx in range(4 ** d):
                part = idx << (2 * (log2 - 2))
                out[first[d] + idx] = sum(1 << u for u, f in enumerate(_units(lg, _zx(part), _zy(part), 1 << log2, part, edge)) if f)
        return out
    if lg <= 5: assert np.array_equal(table(False), causal_avail(lg))  # (a 64x64 CU's root has 33 units: causal_avail cannot build its table)
    return table(True)


def _rough_flags(lg, nxn):
    """hop_intra_search_job.rough_flags: the same per PU, a byte per unit"""
    from test_gpu_intra_final_pass import _zx, _zy
    fl = np.zeros((4, 68), np.uint8); N = (1 << lg) >> nxn; parts = 1 << (2 * (lg - 2))
    for pu in range(4 if nxn else 1):
        part = pu * (parts >> 2)
        f = _units(lg, _zx(part), _zy(part), N, part); fl[pu, :len(f)] = f
    return fl


def _content(rng, cu, content, strong):
    """original and prediction of one CU (luma, and the two chroma blocks), noisy or flat; strong: the largest amplitude (the first candidate of a class, so that a class
    of one candidate has levels too)"""
    pred = [np.full((cu, cu), 128, np.int16), np.full((cu // 2, cu // 2), 128, np.int16), np.full((cu // 2, cu // 2), 128, np.int16)]
    org = [p.copy() for p in pred]
    if content == "noisy":
        yy, xx = np.mgrid[0:cu, 0:cu]; amp = float(rng.choice([4, 12, 40])) if not strong else 40.0
        r = amp * np.sin(xx * rng.uniform(0.1, 0.9) + rng.uniform(0, 3)) * np.cos(yy * rng.uniform(0.1, 0.9)) + rng.normal(0, amp / 4, (cu, cu))
        m = rng.random((cu, cu)) < 0.06; r[m] += rng.choice([-1, 1], int(m.sum())) * 6 * amp
        org[0] = np.clip(org[0] + np.rint(r), 0, 255).astype(np.int16)
        for k in (1, 2): org[k] = np.clip(org[k] + np.rint(r[::2, ::2] * (0.5 if k == 1 else -0.4)), 0, 255).astype(np.int16)
    return org, pred


def _case(hp, side, lg, nxn, n, content):
    """n candidates of one class, candidate t at (64, 64) of picture t of the stack: planes, job records, coder states"""
    L = hp.load(); L.hop_cabac_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]; L.hop_cabac_cu_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    rng = np.random.default_rng(1000 * lg + 100 * nxn + 10 * n + (side == "intra"))
    cu = 1 << lg
    org = [[np.full((H >> (k > 0), W >> (k > 0)), 128, np.int16) for _ in range(PICS)] for k in range(3)]
    pred = [[a.copy() for a in org[k]] for k in range(3)]
    # the reconstruction around the CUs: what intra prediction reads (noisy: coding noise on a smooth ramp; flat: the flat picture itself)
    rec = [[a.copy() for a in org[k]] for k in range(3)]
    jobs = np.zeros(n, hp.RQT_JOB_DTYPE); snaps = np.zeros((n, hp.CABAC_CTX_BYTES), np.uint8); cus = np.zeros((n, hp.CABAC_CU_CTX_BYTES), np.uint8)
    ctx0 = hp.Context(W, H, pictures=PICS); pitch = ctx0.pitch; ctx0.close()
    qps = []
    for t in range(n):
        o, p = _content(rng, cu, content, t == 0)
        for k in range(3):
            s = 1 if k else 0
            org[k][t][Y0 >> s:(Y0 + cu) >> s, X0 >> s:(X0 + cu) >> s] = o[k]
            pred[k][t][Y0 >> s:(Y0 + cu) >> s, X0 >> s:(X0 + cu) >> s] = p[k]
            if content == "noisy":
                ramp = 128 + (np.arange(W >> s)[None, :] - (X0 >> s)) // 2 + (np.arange(H >> s)[:, None] - (Y0 >> s)) // 3
                rec[k][t] = np.clip(ramp + rng.integers(-3, 4, ramp.shape), 0, 255).astype(np.int16)
        if side == "intra" and content == "noisy":                       # an intra CU's original continues its surroundings, plus the noisy residual
            for k in range(3):
                s = 1 if k else 0
                blk = rec[k][t][Y0 >> s:(Y0 + cu) >> s, X0 >> s:(X0 + cu) >> s].astype(np.int32) + (o[k].astype(np.int32) - 128)
                org[k][t][Y0 >> s:(Y0 + cu) >> s, X0 >> s:(X0 + cu) >> s] = np.clip(blk, 0, 255).astype(np.int16)
        qp = int(rng.integers(22, 40)) if t else 24
        lam = 0.57 * 2.0 ** ((qp - 12) / 3.0); w = float(rng.choice([1.0, 1.26])); qps.append(qp)
        j = jobs[t]
        j["x"], j["y"], j["log2_cu"], j["qp_scaled"], j["ctx_index"] = X0, t * pitch + Y0, lg, (qp, qp - 1, qp - 2), t
        j["sign_hide"], j["use_ts"], j["log2_max_tu"], j["log2_min_tu_in_cu"] = 1, 1, 5, max(2, lg - 2)
        j["lambda_rd"], j["lambda_rdoq"], j["dist_weight"] = lam, (lam, lam / w, lam / w), (w, w)
        assert L.hop_cabac_init(snaps[t].ctypes.data, int(rng.integers(0, 5)), qp) == 0 and L.hop_cabac_cu_init(cus[t].ctypes.data, int(rng.integers(0, 5)), qp) == 0
        left = int(rng.integers(0, 32768)); snaps[t, 150], snaps[t, 151] = left & 255, left >> 8
    C = dict(side=side, lg=lg, nxn=nxn, n=n, org=org, pred=pred, rec=rec, jobs=jobs, snaps=snaps, cus=cus)
    if side == "inter":
        syn = np.zeros(n, hp.CU_SYNTAX_DTYPE)
        for t in range(n):
            s = syn[t]; s["n_pu"], s["max_merge_cand"], s["amp_acc"], s["is_min_cu"], s["skip_ctx"] = 1, 5, int(cu >= 16), int(cu == 8), int(rng.integers(0, 3))
            s["pu"][0]["mvd"] = rng.integers(-40, 41, 2); s["pu"][0]["gt_flag"] = int(rng.integers(0, 2)); s["pu"][0]["gt"] = rng.integers(-3, 4, 8)
        C["syn"] = syn
    else:
        syn = np.zeros(n, hp.INTRA_CU_SYNTAX_DTYPE); opts = np.zeros(n, hp.INTRA_RQT_OPT_DTYPE); sj = np.zeros(n, hp.INTRA_SEARCH_JOB_DTYPE)
        sj["left_dir"] = rng.integers(0, 35, (n, 4)); sj["above_dir"] = rng.integers(0, 35, (n, 4)); sj["rough_flags"] = _rough_flags(lg, nxn)
        av = _causal_avail(lg)
        for t in range(n):
            s = syn[t]
            s["part_nxn"], s["skip_flag"], s["skip_ctx"], s["is_min_cu"] = nxn, 0, int(rng.integers(0, 3)), int(lg == 3)
            s["luma_dir"] = rng.integers(0, 35, 4)
            for p in range(4): s["preds"][p] = rng.choice(35, 3, replace=False); s["pred_num"][p] = 3
            s["chroma_is_dm"], s["chroma_dir"], s["tr_depth"], s["part"], s["b_luma"] = 1, 36, nxn, 0, 1
            opts[t]["check_first"], opts[t]["ts_fast"], opts[t]["strong"] = 0, int(rng.random() < 0.3), int(rng.integers(0, 2))
            opts[t]["avail"] = av
            sj[t]["sqrt_lambda"] = float(np.sqrt(jobs[t]["lambda_rd"])); sj[t]["num_full_rd"] = 8 if (cu >> nxn) <= 8 else 3
        C["syn"], C["opts"], C["sj"] = syn, opts, sj
    return C


def _run(hp, cls, n, content, form_env, fill=None):
    """one class through its *_device_classes entry in one form: {output name: bytes}, the context's reconstruction planes among them"""
    key = (cls, n, content, tuple(sorted(form_env.items())), fill)
    if key in _runs: return _runs[key]
    import torch
    side, lg, nxn = cls
    ck = ("case", cls, n, content)
    if ck not in _runs: _runs[ck] = _case(hp, side, lg, nxn, n, content)
    C = _runs[ck]
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    cu = 1 << lg
    settings = dict(form_env)
    if fill is not None: settings["HOP_WALK_FILL"] = str(fill)
    with _env(settings):
        ctx = hp.Context(W, H, pictures=PICS)                               # (HOP_WALK is read when a context is created, the other switches per call)
        try:
            ctx.upload_orig(*[ctx.stack(C["org"][k], chroma=k > 0) for k in range(3)])
            for k in range(3):
                ctx.plane_upload("pred", k, ctx.stack(C["pred"][k], chroma=k > 0)); ctx.plane_upload("recon", k, ctx.stack(C["rec"][k], chroma=k > 0))
            d_snap = up(C["snaps"]); d_cus = up(C["cus"])
            if side == "inter":
                CLS = np.dtype([("n", "<i4"), ("pad", "<i4"), ("cls", hp.RQT_JOB_DTYPE)] + [(k, "<u8") for k in ("d_jobs", "d_syntax") + INTER_OUT])
                bufs = dict(d_jobs=up(C["jobs"]), d_syntax=up(C["syn"]), d_results=z(n * hp.RQT_RESULT_DTYPE.itemsize), d_coef=z(n * cu * cu * 3 // 2 * 4), d_ctx_after=z(n * hp.CABAC_CTX_BYTES),
                            d_finals=z(n * 16), d_bits=z(n * 4), d_skipped=z(n * 4), d_cost=z(n * 8), d_ctx_out=z(n * hp.CABAC_CTX_BYTES), d_cu_ctx_out=z(n * hp.CABAC_CU_CTX_BYTES))
                desc = np.zeros(1, CLS); desc[0]["n"], desc[0]["cls"] = n, C["jobs"][0]
                entry, names = "hop_inter_cu_device_classes", INTER_OUT
            else:
                CLS = np.dtype([("n", "<i4"), ("part_nxn", "<i4"), ("num_full_rd", "<i4"), ("pad", "<i4"), ("cls", hp.RQT_JOB_DTYPE)] + [(k, "<u8") for k in
                               ("d_jobs", "d_syntax", "d_opts", "d_sjobs") + INTRA_OUT])
                bufs = dict(d_jobs=up(C["jobs"]), d_syntax=up(C["syn"]), d_opts=up(C["opts"]), d_sjobs=up(C["sj"]),
                            d_sresults=z(n * hp.INTRA_SEARCH_RESULT_DTYPE.itemsize), d_results=z(n * hp.RQT_RESULT_DTYPE.itemsize), d_cresults=z(n * 8), d_coef=z(n * cu * cu * 3 // 2 * 4),
                            d_reco_y=z(n * cu * cu * 2), d_reco_c=z(n * cu * cu // 2 * 2), d_syntax_out=z(n * hp.INTRA_CU_SYNTAX_DTYPE.itemsize), d_dist=z(n * 4), d_bits=z(n * 4),
                            d_cost=z(n * 8), d_ctx_out=z(n * hp.CABAC_CTX_BYTES), d_cu_ctx_out=z(n * hp.CABAC_CU_CTX_BYTES))
                desc = np.zeros(1, CLS); desc[0]["n"], desc[0]["part_nxn"], desc[0]["num_full_rd"], desc[0]["cls"] = n, nxn, int(C["sj"][0]["num_full_rd"]), C["jobs"][0]
                entry, names = "hop_intra_cu_device_classes", INTRA_OUT
            for name, t in bufs.items(): desc[0][name] = t.data_ptr()
            fn = getattr(ctx.L, entry); fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            ctx._chk(fn(ctx.h, 1, desc.ctypes.data, d_snap.data_ptr(), d_cus.data_ptr()), entry)
            ctx.sync()
            got = {name: bufs[name].cpu().numpy().tobytes() for name in names}
            for k in range(3): got["recon%d" % k] = ctx.recon_download(k).tobytes()
        finally:
            ctx.close()
    _runs[key] = got
    return got


def _ident(cls): return "%s-%d%s" % (cls[0], 1 << cls[1], "-NxN" if cls[2] else "")


@pytest.mark.parametrize("content", ["noisy", "flat"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cls", CLASSES, ids=_ident)
def test_walk_forms_give_the_staged_chain_byte_for_byte(hp, cls, n, content):
    """results, levels, coder states, bits, distortions, syntax out and the context's three planes: the side-by-side walk and the one-after-the-other walk against the batch steps"""
    ref = _run(hp, cls, n, content, FORMS[2][1])
    for form, env in FORMS[:2]:
        got = _run(hp, cls, n, content, env)
        for name in ref:
            assert got[name] == ref[name], (_ident(cls), n, content, form, "differs from the batch steps in", name)
    # the case is what it says: a flat picture has no level, a noisy one has some, and a cost came out
    coef = np.frombuffer(ref["d_coef"], np.int32)
    assert (np.frombuffer(ref["d_cost"], np.float64) > 0).all()
    if content == "flat": assert not coef.any()
    else: assert coef.any()


@pytest.mark.parametrize("content", ["noisy", "flat"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cls", FILL_CLASSES, ids=_ident)
def test_walk_results_do_not_depend_on_what_the_work_buffer_held(hp, cls, n, content):
    """HOP_WALK_FILL unset, 0 and 255: the same bytes in every output"""
    ref = _run(hp, cls, n, content, {})
    for fill in (0, 255):
        got = _run(hp, cls, n, content, {}, fill)
        for name in ref:
            assert got[name] == ref[name], (_ident(cls), n, content, "HOP_WALK_FILL=%d" % fill, "changes", name)


@pytest.mark.parametrize("bad", ["abc", "12x", "256", "-1"])
def test_walk_fill_takes_a_byte_value_only(hp, bad):
    """anything but a decimal 0..255 is an error of the call, not a fill with whatever the digits in front give"""
    with pytest.raises(hp.HopError, match="HOP_WALK_FILL"):
        _run(hp, ("inter", 3, 0), 1, "flat", {}, bad)
