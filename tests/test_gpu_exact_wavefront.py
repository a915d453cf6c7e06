"""GPU: hop_encode_set_exact -- the exact wavefront.  At lag 2 (the least distance between two CTU rows at which a CTU's neighbour above and to the right is coded) a
plain wavefront is far from raster order: almost every search of a row >= 1 reaches columns of the row above that are not coded yet, and the rows below are partly coded
where the reference has nothing.  In exact mode the decisions must still be the reference encoder's own, candidate by candidate (the goldens of the WaveFrontSynchro
runs), because the rows below are kept out of sight by the kernels (hop_ctx_set_row_limit) and the rows above are waited for."""
import os
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

from hoputil import ROOT, lenslet
from test_exact_wait_column import BOUND_H, BOUND_W, bound_jobs, reach_above
from test_spine_cpu import RAGGED, check_against_golden, frame, ragged_golden, ragged_picture

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

pytestmark = pytest.mark.gpu

LAG = 2
_npz = {}


def golden(name):
    if name == "ragged": return ragged_golden()
    if name not in _npz:
        with np.load(os.path.join(ROOT, "tests", "golden", name)) as z: _npz[name] = {k: z[k] for k in z.files}
    return _npz[name]


# key, golden file, W, H, MIsize (= lenslet pitch), the picture
PICTURES = {
    "448x192_seed3_wpp":      ("encoder_spine.npz", 448, 192, 16, lambda: frame(448, 192, 3, False)),
    "192x128_seed7_wpp":      ("encoder_spine.npz", 192, 128, 16, lambda: frame(192, 128, 7, False)),
    "448x192_seed3_mi15_wpp": ("encoder_spine_mi15.npz", 448, 192, 15, lambda: lenslet(448, 192, 15, 3)),
    RAGGED[0][0]:             ("ragged", 432, 184, 16, lambda: ragged_picture(16)),
}


def plain(parts):
    return parts.view(np.dtype(parts.dtype.descr))


def encode(ctx, mi, lag=LAG, trace=True):
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        out = ctx.encode_frame(32, mi, 0, tp if trace else None, wpp=1, wavefront_lag=lag)
        n = ctx.pictures
        text = [open(tp + (".%d" % k if n > 1 else ""), "rb").read() for k in range(n)] if trace else None
    return out, text


@pytest.mark.parametrize("slots", [0, 48])
@pytest.mark.parametrize("key", list(PICTURES))
def test_exact_wavefront_at_lag_2_equals_the_reference_encoder(key, slots):
    """costs, bits, distortions, partition data and the candidate trace against the reference's own run; no search may be counted as reaching uncoded samples above (the
    visibility check runs after the wait), and on the 448-wide pictures rows must have waited.

    searches_reaching_below -- the searches the row limit protected -- is printed and NOT asserted: on an MI355X it is 0 for all four pictures and both slot settings
    (448x192: 4 / 31 waits at 0 / 48 slots; 192x128: 1 / 10; 448x192 --MIsize=15: 4 / 33; 432x184: 5 / 34).  That is what the waits do on pictures this narrow: a search
    of CTU c waits for column c + 3 of the row above, so a row runs at least 4 CTUs behind the row above it, while a window of +-128 samples around an ordinary predictor
    reaches 3 CTUs to the left -- the row below has coded nothing inside it.  With the mode off at lag 2 the same picture counts 1 300 such searches (test_the_hazard_is_real)."""
    gname, W, H, mi, pic = PICTURES[key]
    ctx = hp.Context(W, H, slots=slots)
    ctx.upload_orig(*pic())
    ctx.set_exact(1)
    (cost, bits, dist, parts, nc), text = encode(ctx, mi)
    rv = ctx.encode_stats()["rendezvous"]
    print(key, "slots", slots, {k: rv[k] for k in ("rounds", "requests", "searches_reaching_below", "searches_reaching_above", "waits", "wait_ms")})
    check_against_golden(golden(gname), key, cost, bits, dist, plain(parts), text[0])
    assert ctx.encode_progress() == len(cost)
    if W == 448:
        assert rv["searches_reaching_above"] == 0 and rv["waits"] > 0, rv
    else:
        assert rv["searches_reaching_above"] == 0, rv
    # the limit was the call's: the context is back to what it was
    q = np.array([(0, 0, 16, 16, 0, 4 * 60)], np.int32)
    assert ctx.valid_pattern(q)[0] == 1                                  # (a probe below CTU row 0 finds the coded picture again)
    ctx.close()


def test_the_hazard_is_real():
    """the same picture at lag 2 with the mode off: searches reach columns of the row above that are not coded (whether that changes a decision on this picture is printed,
    not asserted: the count is what the mode answers)"""
    key = "448x192_seed3_wpp"
    gname, W, H, mi, pic = PICTURES[key]
    ctx = hp.Context(W, H, slots=48)
    ctx.upload_orig(*pic())
    (cost, bits, dist, parts, nc), _ = encode(ctx, mi, trace=False)
    rv = ctx.encode_stats()["rendezvous"]
    G = golden(gname)
    print("lag 2, exact off:", {k: rv[k] for k in ("searches_reaching_below", "searches_reaching_above", "waits")}, "CTUs whose cost differs from the reference:",
          int((cost != G[key + "/cost"]).sum()), "of", len(cost))
    assert rv["searches_reaching_above"] > 0 and rv["waits"] == 0
    assert rv["searches_reaching_below"] > 0        # (the row below runs 2 CTUs behind, a window reaches 3 to the left: certain -- and what the row limit is for)
    ctx.close()


def test_a_stack_in_exact_mode_codes_every_picture_as_raster_order_does():
    """three 192x128 pictures in one stacked context, exact, lag 2: picture 0 against the reference's golden, the others against contexts of their own coded with
    wavefront_lag = 3 = the number of columns, which is raster order on the existing path; reconstruction and SS reference too"""
    W, H = 192, 128
    pics = [frame(W, H, 7, False), frame(W, H, 8, False), frame(W, H, 11, False)]
    ctx = hp.Context(W, H, pictures=3, slots=16)
    ctx.upload_orig(ctx.stack([p[0] for p in pics]), ctx.stack([p[1] for p in pics], True), ctx.stack([p[2] for p in pics], True))
    ctx.set_exact(1)
    (cost, bits, dist, parts, nc), text = encode(ctx, 16)
    rv = ctx.encode_stats()["rendezvous"]
    assert rv["searches_reaching_above"] == 0, rv
    n = 6
    check_against_golden(golden("encoder_spine.npz"), "192x128_seed7_wpp", cost[:n], bits[:n], dist[:n], plain(parts)[:n], text[0])
    rec = [ctx.unstack(ctx.recon_download(c), c > 0) for c in range(3)]
    ss = ctx.ssref_download(0)
    for k, (Y, Cb, Cr) in enumerate(pics):
        one = hp.Context(W, H, slots=16)
        one.upload_orig(Y, Cb, Cr)
        c1, b1, d1, p1, _ = one.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=3)
        assert np.array_equal(cost[k * n:(k + 1) * n], c1) and np.array_equal(bits[k * n:(k + 1) * n], b1) and np.array_equal(dist[k * n:(k + 1) * n], d1), k
        assert parts[k * n:(k + 1) * n].tobytes() == p1.tobytes(), k
        for c in range(3):
            assert np.array_equal(rec[c][k], one.recon_download(c)), (k, c)
        assert np.array_equal(ss[k * ctx.pitch:k * ctx.pitch + H + 160], one.ssref_download(0)), k
        one.close()
    ctx.close()


def _coded(ctx):
    return [ctx.recon_download(c) for c in range(3)] + [ctx.ssref_download(0), ctx.levels_download()]


@pytest.mark.parametrize("W,H,plain_intra,slots", [(384, 384, 1, 0), (192, 384, 0, 48)])
def test_more_rows_than_lanes(W, H, plain_intra, slots):
    """Row r works on lane r % rif (stash slots, levels), rif = ceil(columns / lag) + 1.  The progress gate alone lets row r + rif start while row r is still coding: over k
    rows only k (lag - 1) + 1 retired CTUs are certain.  384x384 plain intra at lag 2: 6 columns, rif 4, no searches and so no waits -- the rows run 2 CTUs apart and row 4
    is let on when row 0 is certain of 5 of its 6 CTUs; 192x384 HOP: 3 columns, rif 3, 6 rows.  A row therefore waits for the row rif above it to END, and two rows on one
    lane are an error (hop_encode_frame fails) instead of a silently wrong reconstruction.  Against the same picture in raster order: wavefront_lag = the number of columns."""
    Y, Cb, Cr = lenslet(W, H, 16, 31)
    cols = W // 64
    ctx = hp.Context(W, H, slots=slots); ctx.upload_orig(Y, Cb, Cr); ctx.set_exact(1)
    got = ctx.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=LAG, plain_intra=plain_intra)
    rv = ctx.encode_stats()["rendezvous"]
    assert ctx.encode_progress() == len(got[0]) == cols * (H // 64) and (got[0] > 0).all()
    got_planes = _coded(ctx)
    ctx.close()
    ref = hp.Context(W, H, slots=slots); ref.upload_orig(Y, Cb, Cr)
    want = ref.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=cols, plain_intra=plain_intra)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b), np.nonzero(a != b)[0][:8]
    assert got[3].tobytes() == want[3].tobytes()
    for k, (a, b) in enumerate(zip(got_planes, _coded(ref))):
        assert np.array_equal(a, b), k
    print("%dx%d plain_intra %d:" % (W, H, plain_intra), rv["rounds"], "rounds,", rv["requests"], "requests,", rv["waits"], "waits")
    if plain_intra: assert rv["requests"] > 1.3 * rv["rounds"]          # (no waits, rows 2 CTUs apart and in step: they did run side by side)
    ref.close()


def test_cancel_in_exact_mode_reports_only_finished_ctus():
    """hop_encode_cancel releases the rows that wait for a row above which will not go on; a CTU given up that way is never reported as coded"""
    key = "448x192_seed3_wpp"
    gname, W, H, mi, pic = PICTURES[key]
    G = golden(gname)
    ctx = hp.Context(W, H, slots=48)
    ctx.upload_orig(*pic())
    ctx.set_exact(1)
    out = {}
    th = threading.Thread(target=lambda: out.update(r=ctx.encode_frame(32, mi, 0, None, wpp=1, wavefront_lag=LAG)))
    th.start()
    while th.is_alive() and ctx.encode_progress() < 3: time.sleep(0.005)
    ctx.encode_cancel(); th.join()
    cost, bits, dist = out["r"][:3]
    done = cost > 0
    print("cancelled after", int(done.sum()), "of", len(cost), "CTUs")
    assert 3 <= int(done.sum()) == ctx.encode_progress() < len(cost)
    assert np.array_equal(cost[done], G[key + "/cost"][done]) and np.array_equal(bits[done], G[key + "/bits"][done]) and np.array_equal(dist[done], G[key + "/dist"][done])
    assert not bits[~done].any() and not dist[~done].any()
    # every row's finished CTUs are its first ones
    cols = (W + 63) // 64
    for r in range((H + 63) // 64):
        d = done[r * cols:(r + 1) * cols]
        assert not d[int(d.sum()):].any(), (r, d)
    ctx.close()


def test_what_exact_mode_refuses_and_what_it_ignores(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hop_shard", os.path.join(ROOT, "hevc-hop_amd", "shard.py"))
    sh = importlib.util.module_from_spec(spec); spec.loader.exec_module(sh)
    W, H = 128, 64
    Y, Cb, Cr = lenslet(W, H, 16, 12)

    def refused(ctx, what, **kw):
        with pytest.raises(hp.HopError) as e:
            ctx.encode_frame(32, 16, 0, None, wpp=1, **kw)
        assert e.value.code == -1 and "exact" in str(e.value), (what, str(e.value))           # HOP_ERR_ARG, with a message that names the mode
    ctx = hp.Context(W, H); ctx.upload_orig(Y, Cb, Cr); ctx.set_exact(1)
    refused(ctx, "streams", wavefront_lag=2, streams=2)
    refused(ctx, "lag", wavefront_lag=1)
    ag = sh.ThreadAllgather(2, timeout=5.0)
    ctx.set_shard(0, 2, ag.rank(0))
    refused(ctx, "shard", wavefront_lag=2)
    ctx.set_shard(0, 1, None)
    st = hp.Context(W, H, pictures=2); st.upload_orig(st.stack([Y, Y]), st.stack([Cb, Cb], True), st.stack([Cr, Cr], True)); st.set_exact(1)
    monkeypatch.setenv("HOP_SPINE_GROUPS", "2")
    refused(st, "groups", wavefront_lag=2)
    monkeypatch.delenv("HOP_SPINE_GROUPS")
    st.close()
    # raster order ignores the switch; and the setter, once called, outranks the environment either way
    want = ctx.encode_frame(32, 16, 0, None, wpp=1)
    ctx.set_exact(0)
    monkeypatch.setenv("HOP_ENCODE_EXACT", "1")
    got = ctx.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=1)       # (exact mode would refuse lag 1)
    for a, b in zip(want[:3], got[:3]):
        assert np.array_equal(a, b)
    ctx.close()
    fresh = hp.Context(W, H); fresh.upload_orig(Y, Cb, Cr)                # never told: the environment decides
    refused(fresh, "lag, by the environment", wavefront_lag=1)
    got = fresh.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=2)
    for a, b in zip(want[:3], got[:3]):
        assert np.array_equal(a, b)
    monkeypatch.setenv("HOP_ENCODE_EXACT", "0")
    fresh.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=1)
    fresh.close()


def test_a_search_reads_nothing_of_the_row_above_beyond_the_column_the_spine_waits_for():
    """a dozen PUs of CTU row 1 over random planes: every CTU of row 0 beyond the column hop_me_reach_above names is overwritten with the sentinel, one at a time -- the GT-stage
    result of the search must not change.  (That the searches do read row 0: with the whole row overwritten every one of them changes.)"""
    W, H = BOUND_W, BOUND_H
    rng = np.random.default_rng(17)
    A = [rng.integers(0, 256, (H + 160, W + 160)).astype(np.int16), rng.integers(0, 256, (H // 2 + 80, W // 2 + 80)).astype(np.int16), rng.integers(0, 256, (H // 2 + 80, W // 2 + 80)).astype(np.int16)]
    ctx = hp.Context(W, H)
    ctx.upload_orig(*lenslet(W, H, 16, 3))
    for c in range(3): ctx.ssref_upload(c, A[c])
    jobs = bound_jobs()
    cols = np.array([reach_above(ctx.L, W, j, 64) for j in jobs])
    assert cols.min() >= 0 and (cols < 6).sum() >= 6
    base = ctx.me_search(jobs, hp.HOP_STAGE_GT)
    assert not base["not_valid"].any()

    def same(a, b):
        return all(np.array_equal(a[n], b[n]) for n in hp.PU_RESULT_DTYPE.names)
    for cc in range(1, 7):
        B = A[0].copy()
        B[80:80 + 64, 80 + 64 * cc:80 + 64 * (cc + 1)] = -1
        ctx.ssref_upload(0, B)
        got = ctx.me_search(jobs, hp.HOP_STAGE_GT)
        for i in np.nonzero(cols < cc)[0]:
            assert same(got[i:i + 1], base[i:i + 1]), (int(i), int(cols[i]), cc, got[i], base[i])
    B = A[0].copy(); B[80:80 + 64, 80:80 + W] = -1
    ctx.ssref_upload(0, B)
    got = ctx.me_search(jobs, hp.HOP_STAGE_GT)
    assert not any(same(got[i:i + 1], base[i:i + 1]) for i in range(len(jobs)))
    ctx.close()
