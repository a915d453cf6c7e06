"""GPU: hop_ctx_set_row_limit -- raster-order visibility for every kernel that reads the SS reference (k_ss_search / k_ss_family, k_frac, k_gt_search, the inter
predictor behind hop_pred_inter, k_valid_pattern).

In raster order a CTU of row k finds every sample whose picture row is >= 64 (k + 1) still holding the sentinel, margin samples that copy such a row included.  The
kernels must behave as if that were so WITHOUT the samples being touched.  The reference for "as if" needs no second implementation: plane set A is random samples
without a sentinel; plane set B(k) is A with exactly those rows overwritten by -1.  The limit on over A must give, field for field, what the limit off gives over B(k).
The picture is 200x184: three CTU rows, partial CTUs on the right (8 wide) and below (56 tall)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from hoputil import ROOT, lambda_for_qp, lenslet

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 200, 184
MY, MC = 80, 40                          # the SS reference's margins
LAM = lambda_for_qp(32)[1]
FLAGS = hp.HOP_FLAG_FEN | hp.HOP_FLAG_HADME
SHAPES = [(64, 64), (32, 64), (64, 16), (16, 16), (8, 4)]


def planes_a(w, h, seed):
    """three padded SS planes of random reconstructed-looking samples (0..255): nothing in them is the sentinel"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h + 2 * MY, w + 2 * MY)).astype(np.int16),
            rng.integers(0, 256, (h // 2 + 2 * MC, w // 2 + 2 * MC)).astype(np.int16),
            rng.integers(0, 256, (h // 2 + 2 * MC, w // 2 + 2 * MC)).astype(np.int16)]


def planes_b(A, limit, top=0, ph=H):
    """A with every padded row whose source picture row -- itself, or for a margin row the nearest row of the picture that starts at `top` and is `ph` tall -- is >= limit
    set to the sentinel.  Rows above `top` belong to another picture of a stack and stay."""
    B = [a.copy() for a in A]
    for c, (b, m) in enumerate(zip(B, (MY, MC, MC))):
        t, p, lim = (top, ph, limit) if c == 0 else (top // 2, ph // 2, limit // 2)
        y = np.arange(b.shape[0]) - m                                   # picture row of every padded row
        src = np.clip(y, t, t + p - 1)
        b[(src >= lim) & (y >= t)] = -1
    return B


def upload(ctx, planes):
    for c, p in enumerate(planes):
        ctx.ssref_upload(c, p)


def pu_job(x, y, w, h, pred, amvp, rng=(-40, 24, -8, 40)):
    j = np.zeros(1, hp.PU_JOB_DTYPE)[0]
    j["pu_x"], j["pu_y"], j["w"], j["h"] = x, y, w, h
    j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"] = rng
    j["off_x"], j["off_y"] = 1000, 1000                                 # (the rule of TEncSearch.cpp:6328 rejects nothing: the window may lie below the PU)
    j["pred_x"], j["pred_y"], j["lambda_cost"], j["n_amvp"] = pred[0], pred[1], LAM, len(amvp) // 2
    j["amvp"] = list(amvp) + [0] * (4 - len(amvp))
    j["flags"] = FLAGS
    return j


def search_jobs(k, top=0):
    """PUs at the bottom of CTU row k: the five shapes, and the five symmetric PUs of one 32x32 CU in the order that makes them a family (k_ss_family).  Predictor and
    AMVP vectors point down and down-left, so the search windows, the fractional taps and the GT patches around every start vector cross the limit 64 (k + 1)."""
    bot = top + 64 * (k + 1)
    jobs = []
    for i, (w, h) in enumerate(SHAPES):
        jobs.append(pu_job(64 + 4 * i, bot - h, w, h, (-80, 96), (-80, 96, -160, 64)))
        jobs.append(pu_job(128, bot - h, w, h, (0, 40), (0, 40, -24, 120)))
    cy = bot - 32
    for (ox, oy, w, h) in ((0, 0, 32, 32), (0, 0, 16, 32), (16, 0, 16, 32), (0, 0, 32, 16), (0, 16, 32, 16)):
        jobs.append(pu_job(96 + ox, cy + oy, w, h, (-40, 60), (-40, 60, 16, 100)))
    return np.array(jobs, hp.PU_JOB_DTYPE)


_state = {}


def fixtures():
    """one context over A (the limit is switched per test and always left off), one over B(k) per CTU row, the planes and the original: made once"""
    if not _state:
        Y, Cb, Cr = lenslet(W, H, 16, 21)
        A = planes_a(W, H, 5)
        ca = hp.Context(W, H); ca.upload_orig(Y, Cb, Cr); upload(ca, A)
        cb = []
        for k in range(3):
            c = hp.Context(W, H); c.upload_orig(Y, Cb, Cr); upload(c, planes_b(A, 64 * (k + 1))); cb.append(c)
        _state.update(Y=Y, A=A, ca=ca, cb=cb)
    return _state


def same_results(a, b, what):
    for name in hp.PU_RESULT_DTYPE.names:
        assert np.array_equal(a[name], b[name]), (what, name, np.argwhere(a[name] != b[name])[:8].tolist())


@pytest.mark.parametrize("wide", ["0", "2"])          # HOP_ME_WIDE: the size-class form and the one-launch form of the fractional and the GT search
@pytest.mark.parametrize("stage", [hp.HOP_STAGE_INT, hp.HOP_STAGE_FRAC, hp.HOP_STAGE_GT])
@pytest.mark.parametrize("k", [0, 1])
def test_search_with_the_limit_equals_the_search_over_masked_planes(k, stage, wide, monkeypatch):
    monkeypatch.setenv("HOP_ME_WIDE", wide)
    S = fixtures()
    jobs = search_jobs(k)
    want = S["cb"][k].me_search(jobs, stage)
    S["ca"].set_row_limit(1)
    try: got = S["ca"].me_search(jobs, stage)
    finally: S["ca"].set_row_limit(0)
    same_results(got, want, (k, stage, wide))
    off = S["ca"].me_search(jobs, stage)
    assert not all(np.array_equal(off[n], want[n]) for n in hp.PU_RESULT_DTYPE.names), "the jobs do not reach the limit: the comparison shows nothing"
    assert int((want["not_valid"] == 0).sum()) >= len(jobs) // 2          # (and most of the searches still find a vector above it)


def pred_jobs(k, top=0):
    """all 16 quarter-sample phases, GT off and on, blocks that end above, straddle and lie below the limit 64 (k + 1) of the PU's CTU row.  A list of requests: the jobs of
    one request write disjoint rectangles of the prediction picture"""
    bot = top + 64 * (k + 1)
    calls = []
    for ph in range(16):
        fx, fy = ph & 3, ph >> 2
        for gt in (0, 1):
            jobs = []
            for (w, h, x, dy) in ((16, 16, 64, 6), (32, 8, 96, -3), (8, 8, 48, 20), (64, 64, 128, 30)):
                y = bot - h
                jobs.append(hp.PredJob(x, y, w, h, 4 * (ph - 8) + fx, 4 * dy + fy, gt, (ctypes.c_int32 * 8)(*([1, -2, 2, 1, -1, 2, -2, -1] if gt else [0] * 8)), 0))
            calls.append(jobs)
    return calls


def predict(ctx, calls):
    out = [ctx.pred_inter(jobs) for jobs in calls]
    return [np.concatenate([o[c] for o in out]) for c in range(3)]


@pytest.mark.parametrize("k", [0, 1])
def test_prediction_with_the_limit_equals_the_prediction_over_masked_planes(k):
    S = fixtures()
    calls = pred_jobs(k)
    want = predict(S["cb"][k], calls)
    S["ca"].set_row_limit(1)
    try: got = predict(S["ca"], calls)
    finally: S["ca"].set_row_limit(0)
    off = predict(S["ca"], calls)
    for c, name in enumerate(("Y", "Cb", "Cr")):
        assert np.array_equal(got[c], want[c]), (k, name, np.nonzero(got[c] != want[c])[0][:8])
        assert not np.array_equal(off[c], want[c]), (k, name, "no job reaches the limit")


def test_valid_pattern_with_the_limit_equals_the_probes_over_masked_planes():
    S = fixtures()
    q = []
    for k in (0, 1):
        bot = 64 * (k + 1)
        for (w, h) in SHAPES:
            for mv in ((0, -4 * (h + 8)), (-36, -4 * (h + 4)), (12, -4 * (h + 5)), (-80, 24), (40, -4 * h), (0, 0)):
                q.append((64, bot - h, w, h, mv[0], mv[1]))
    q = np.array(q, np.int32)
    S["ca"].set_row_limit(1)
    try: got = S["ca"].valid_pattern(q)
    finally: S["ca"].set_row_limit(0)
    for k in (0, 1):
        sel = q[:, 1] + q[:, 3] == 64 * (k + 1)
        want = S["cb"][k].valid_pattern(q[sel])
        assert np.array_equal(got[sel], want), (k, got[sel], want)
        assert 0 < int(want.sum()) < int(sel.sum())                     # probes on both sides of the limit
    assert S["ca"].valid_pattern(q).all()                              # A holds no sentinel


def test_a_block_planted_below_the_limit_is_found_without_it_and_never_with_it():
    """teeth by construction: a copy of the PU's original block lies below the limit, inside the search window.  Without the limit the integer search returns that vector
    with SAD 0; with it the samples do not exist"""
    S = fixtures()
    Y = S["Y"]
    ctx = hp.Context(W, H); ctx.upload_orig(Y, *lenslet(W, H, 16, 21)[1:]); upload(ctx, S["A"])
    for k in (0, 1):
        for i, (w, h) in enumerate(SHAPES):
            x, y = 64, 64 * (k + 1) - h
            dx, dy = -24 + 8 * i, h + 6                                 # the copy starts 6 rows below the limit
            A0 = S["A"][0].copy()                                       # (one copy at a time: those of different PUs would overlap)
            A0[MY + y + dy:MY + y + dy + h, MY + x + dx:MY + x + dx + w] = Y[y:y + h, x:x + w]
            ctx.ssref_upload(0, A0)
            jobs = np.array([pu_job(x, y, w, h, (4 * dx, 4 * dy), (4 * dx, 4 * dy), rng=(dx - 16, dx + 16, -8, dy + 8))], hp.PU_JOB_DTYPE)
            r = ctx.me_search(jobs, hp.HOP_STAGE_INT)[0]
            assert (int(r["mv_int"][0]), int(r["mv_int"][1]), int(r["sad"]), int(r["not_valid"])) == (dx, dy, 0, 0), (k, w, h, r)
            ctx.set_row_limit(1)
            r = ctx.me_search(jobs, hp.HOP_STAGE_INT)[0]
            ctx.set_row_limit(0)
            # whatever it finds now ends above the limit, its validity probes (4 rows below the block) included: the PU ends AT the limit, so the vector points up by more than 4
            assert int(r["not_valid"]) == 1 or int(r["mv_int"][1]) < -4, (k, w, h, r)
            assert (int(r["mv_int"][0]), int(r["mv_int"][1])) != (dx, dy) and int(r["sad"]) != 0
    ctx.close()


def test_the_last_ctu_row_sees_everything():
    """a PU in the picture's last CTU row: the rows below it are the bottom margin, which copies a row above the limit -- on and off are identical, margin included"""
    S = fixtures()
    jobs = []
    for i, (w, h) in enumerate([(64, 16), (16, 16), (8, 4), (32, 32), (16, 8)]):          # (the row is 56 tall: PUs whose top-left sample lies in it)
        assert H - h >= 128
        jobs.append(pu_job(64 + 4 * i, H - h, w, h, (-80, 96), (-80, 96, -160, 64)))       # windows down to 40 rows below the picture
    jobs = np.array(jobs, hp.PU_JOB_DTYPE)
    pj = [hp.PredJob(64, H - 16, 16, 16, -13, 4 * 30 + 1, gt, (ctypes.c_int32 * 8)(*([1, -2, 2, 1, -1, 2, -2, -1] if gt else [0] * 8)), 0) for gt in (0, 1)]
    q = np.array([(64, H - 16, 16, 16, 0, 40), (64, H - 16, 16, 16, -20, 200)], np.int32)
    off = (S["ca"].me_search(jobs), predict(S["ca"], [pj[:1], pj[1:]]), S["ca"].valid_pattern(q))
    S["ca"].set_row_limit(1)
    try: on = (S["ca"].me_search(jobs), predict(S["ca"], [pj[:1], pj[1:]]), S["ca"].valid_pattern(q))
    finally: S["ca"].set_row_limit(0)
    same_results(on[0], off[0], "last row")
    assert all(np.array_equal(a, b) for a, b in zip(on[1], off[1])) and np.array_equal(on[2], off[2])


def test_a_stacked_context_counts_the_rows_from_the_pictures_own_origin():
    """two 128-row pictures in one context: a PU in picture 1, CTU row 0 -- the limit is that picture's own row 1 (stack row pitch + 64); picture 0's samples, all of them
    above it, stay visible"""
    Ws, Hs = 192, 128
    ctx = hp.Context(Ws, Hs, pictures=2)
    pitch = ctx.pitch
    rng = np.random.default_rng(9)
    org = [rng.integers(0, 256, (ctx.H, Ws)).astype(np.int16), rng.integers(0, 256, (ctx.H // 2, Ws // 2)).astype(np.int16), rng.integers(0, 256, (ctx.H // 2, Ws // 2)).astype(np.int16)]
    ctx.upload_orig(*org)
    A = planes_a(Ws, ctx.H, 6)
    B = planes_b(A, pitch + 64, top=pitch, ph=Hs)
    assert np.array_equal(B[0][:MY + pitch + 64], A[0][:MY + pitch + 64]) and (B[0][MY + pitch + 64:] == -1).all()
    ref = hp.Context(Ws, Hs, pictures=2); ref.upload_orig(*org); upload(ref, B)
    upload(ctx, A)
    jobs = search_jobs(0, top=pitch)
    pj = pred_jobs(0, top=pitch)
    # a search of picture 1 that looks UP, at picture 0's bottom margin: nothing there is limited
    up = np.array([pu_job(64, pitch, 16, 16, (0, -4 * 100), (0, -4 * 100), rng=(-8, 8, -108, -92))], hp.PU_JOB_DTYPE)
    want = (ref.me_search(jobs), predict(ref, pj), ref.me_search(up))
    ctx.set_row_limit(1)
    got = (ctx.me_search(jobs), predict(ctx, pj), ctx.me_search(up))
    ctx.set_row_limit(0)
    off = (ctx.me_search(jobs), predict(ctx, pj), ctx.me_search(up))
    same_results(got[0], want[0], "stack")
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    same_results(got[2], off[2], "stack, upwards"); same_results(got[2], want[2], "stack, upwards")
    assert int(off[2]["not_valid"][0]) == 0
    assert not all(np.array_equal(off[0][n], want[0][n]) for n in hp.PU_RESULT_DTYPE.names)
    ctx.close(); ref.close()


def test_the_decoder_ignores_the_limit():
    """hop_decode_frame on a context with the limit left on: a decoder sees the SS reference as it is"""
    Wd, Hd = 128, 64
    Y, Cb, Cr = lenslet(Wd, Hd, 16, 12)
    e = hp.Context(Wd, Hd); e.upload_orig(Y, Cb, Cr)
    parts = e.encode_frame(32, 16)[3]
    levels = e.levels_download()
    assert int((parts["pred_mode"] == 0).sum()) > 0                     # (SS / GT predicted CUs: their vectors point up and left, their GT patches reach below the PU)
    want = [e.recon_download(c) for c in range(3)]
    d = hp.Context(Wd, Hd)
    d.decode_frame(parts, levels, qp=32)
    off = [d.recon_download(c) for c in range(3)] + [d.ssref_download(c) for c in range(3)]
    d.set_row_limit(1)
    d.decode_frame(parts, levels, qp=32)
    on = [d.recon_download(c) for c in range(3)] + [d.ssref_download(c) for c in range(3)]
    for c in range(6):
        assert np.array_equal(on[c], off[c]), c
    for c in range(3):
        assert np.array_equal(on[c], want[c]), c
    e.close(); d.close()
