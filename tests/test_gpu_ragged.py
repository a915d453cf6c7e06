"""GPU: partial CTUs on the right AND below where things run side by side, and the spine's byte-moving entries on their own.

bench.py's frame (7728x5368: 120 CTU columns + one 48 wide, 83 CTU rows + one 56 tall) and BASELINE config 5 (624x432 views) end in partial CTUs on both edges; the
other wavefront, stack, views, shard and decode tests use multiples of 64.  Here the picture is 432x184 -- the bench frame's remainders in 21 CTUs -- against the
reference encoder's WaveFrontSynchro run AND its reconstruction before the loop filters (tests/golden/encoder_spine_ragged.npz, oracle/make_golden26.py): the lag-5
wavefront with every candidate-slot setting, rows on views, three pictures in a stack, the CTU rows over two contexts (hop_encode_set_shard: both branches of the
backend's import_block), and the decoder.

Then hop_recon_stash, hop_ssref_commit_recon, hop_valid_pattern, hop_recon_put_device and hop_coef_put_device -- which otherwise only run inside hop_encode_frame -- on a
176x120 context (2 CTU columns + 48, 1 CTU row + 56) against plain numpy and the oracle's commit restatement."""
import importlib.util
import os
import sys
import tempfile
import threading

import numpy as np
import pytest

from hoputil import ROOT, Planes, lenslet, oracle, p16
from test_spine_cpu import (RAGGED, RAGGED_H, RAGGED_SEED, RAGGED_W, check_against_golden, check_parts_against_golden, check_recon_against_golden, levels_match_cbf,
                            ragged_golden, ragged_picture)

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, LAG = RAGGED_W, RAGGED_H, 5
COLS, ROWS = (W + 63) // 64, (H + 63) // 64
KEY16 = RAGGED[0][0]
SLOTS = [0, 16, 24, 48]
M = 80                                   # the SS reference's luma margin


def plain(parts):
    return parts.view(np.dtype(parts.dtype.descr))


def recon(ctx):
    return [ctx.recon_download(c) for c in range(3)]


def ssref(ctx):
    return [ctx.ssref_download(c) for c in range(3)]


# ---------------------------------------------------------------- the picture through hop_encode_frame ----------------------------------------------------------------

_across_slots = {}                       # key -> (slots, levels, fraction) of the first setting that ran: every other setting must leave the same


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("key,mi", RAGGED)
def test_wavefront_with_partial_ctus_equals_the_reference(key, mi, slots):
    """lag-5 wavefront whose bottom row is 56 tall and whose last column is 48 wide: candidates, totals, partition data, all three reconstruction planes and the SS
    reference's picture area against the reference encoder; levels consistent with the cbf flags and, with the RD coder's fractions, the same for every slot setting"""
    G = ragged_golden()
    Y, Cb, Cr = ragged_picture(mi)
    ctx = hp.Context(W, H, slots=slots)
    ctx.upload_orig(Y, Cb, Cr)
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        cost, bits, dist, parts, nc = ctx.encode_frame(32, mi, 0, tp, wpp=1, wavefront_lag=LAG)
        text = open(tp, "rb").read()
    check_against_golden(G, key, cost, bits, dist, plain(parts), text)
    check_recon_against_golden(G, key, recon(ctx))
    assert np.array_equal(ctx.ssref_download(0)[M:M + H, M:M + W], G[key + "/rec_y"])
    lv, fr = ctx.levels_download(), ctx.rd_fraction_download()
    assert levels_match_cbf(lv, plain(parts)) > 0 and np.abs(lv).sum() > 0
    first = _across_slots.setdefault(key, (slots, lv, fr))
    assert np.array_equal(lv, first[1]) and np.array_equal(fr, first[2]), (key, slots, "against slots", first[0])
    ctx.close()


def test_wavefront_on_views_with_partial_ctus_equals_the_reference():
    """streams = 4: the wavefront without batching, the three CTU rows on views of their own and one view to spare"""
    G = ragged_golden()
    Y, Cb, Cr = ragged_picture()
    ctx = hp.Context(W, H)
    ctx.upload_orig(Y, Cb, Cr)
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        cost, bits, dist, parts, nc = ctx.encode_frame(32, 16, 0, tp, wpp=1, wavefront_lag=LAG, streams=4)
        text = open(tp, "rb").read()
    check_against_golden(G, KEY16, cost, bits, dist, plain(parts), text)
    check_recon_against_golden(G, KEY16, recon(ctx))
    assert np.array_equal(ctx.ssref_download(0)[M:M + H, M:M + W], G[KEY16 + "/rec_y"])
    ctx.close()


_alone = {}


def alone(seed):
    """the picture of that seed coded in a context of its own (lag-5 wavefront, 16 candidate slots), once per session: what the stacked and the sharded runs must equal"""
    if seed not in _alone:
        Y, Cb, Cr = ragged_picture(16, seed)
        one = hp.Context(W, H, slots=16)
        one.upload_orig(Y, Cb, Cr)
        cost, bits, dist, parts, _ = one.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=LAG)
        _alone[seed] = dict(cost=cost, bits=bits, dist=dist, parts=parts, rec=recon(one), levels=one.levels_download(), fraction=one.rd_fraction_download(), ss=ssref(one))
        one.close()
    return _alone[seed]


@pytest.mark.parametrize("groups", [1, 2])
def test_stacked_pictures_with_partial_ctus_are_coded_as_pictures_of_their_own(groups, monkeypatch):
    """three 432x184 pictures in one stacked context, each ending in a partial CTU row below which it extends ITS margins: picture 0 against the reference's golden, all
    three against contexts of their own -- costs, partition data, reconstruction, levels, fractions and the padded SS plane"""
    monkeypatch.setenv("HOP_SPINE_GROUPS", str(groups))
    G = ragged_golden()
    seeds = [RAGGED_SEED, 4, 5]
    pics = [ragged_picture(16, s) for s in seeds]
    ctx = hp.Context(W, H, pictures=3, slots=16)
    ctx.upload_orig(ctx.stack([p[0] for p in pics]), ctx.stack([p[1] for p in pics], True), ctx.stack([p[2] for p in pics], True))
    n = COLS * ROWS
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        cost, bits, dist, parts, nc = ctx.encode_frame(32, 16, 0, tp, wpp=1, wavefront_lag=LAG)
        text0 = open(tp + ".0", "rb").read()
    check_against_golden(G, KEY16, cost[:n], bits[:n], dist[:n], plain(parts)[:n], text0)
    rec = [ctx.unstack(ctx.recon_download(c), c > 0) for c in range(3)]
    check_recon_against_golden(G, KEY16, [rec[c][0] for c in range(3)])
    levels, fraction = ctx.levels_download(), ctx.rd_fraction_download()
    ss = ctx.ssref_download(0)
    pitch = ctx.pitch
    stats = ctx.encode_stats()
    ctx.close()
    for k, seed in enumerate(seeds):
        one = alone(seed)
        s = slice(k * n, (k + 1) * n)
        assert np.array_equal(cost[s], one["cost"]) and np.array_equal(bits[s], one["bits"]) and np.array_equal(dist[s], one["dist"]), k
        assert parts[s].tobytes() == one["parts"].tobytes(), k
        for c in range(3):
            assert np.array_equal(rec[c][k], one["rec"][c]), (k, c)
        assert np.array_equal(levels[s], one["levels"]) and np.array_equal(fraction[s], one["fraction"]), k
        assert np.array_equal(ss[k * pitch:k * pitch + H + 160], one["ss"][0]), k      # the picture's padded SS plane inside the stack's
    rv = stats["rendezvous"]
    assert rv["requests"] / max(1, rv["rounds"]) > (2.0 if groups == 1 else 1.2)


def test_ctu_rows_with_partial_ctus_over_two_contexts_equal_the_reference():
    """hop_encode_set_shard on 432x184: rank 0 codes rows 0 and 2, rank 1 row 1, so rank 0 imports 64x64 blocks and a 48x64 one, rank 1 the 64x56 blocks of the bottom row
    and the 48x56 corner -- both branches of the backend's import_block.  Both ranks end with the whole picture: the golden's costs and partition data, the reference
    encoder's reconstruction, and all three padded SS planes of a context that coded the picture alone"""
    spec = importlib.util.spec_from_file_location("hop_shard", os.path.join(ROOT, "hevc-hop_amd", "shard.py"))
    sh = importlib.util.module_from_spec(spec); spec.loader.exec_module(sh)
    G = ragged_golden()
    Y, Cb, Cr = ragged_picture()
    ag = sh.ThreadAllgather(2, timeout=300.0)
    ctxs, out, err = [], [None, None], [None, None]
    for k in range(2):
        c = hp.Context(W, H, slots=48); c.upload_orig(Y, Cb, Cr); c.set_shard(k, 2, ag.rank(k)); ctxs.append(c)

    def run(k):
        try: out[k] = ctxs[k].encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=LAG)
        except BaseException as e:
            err[k] = e; ag.barrier.abort()
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    assert err == [None, None], err
    assert [ag.rank(k).calls for k in range(2)] == [COLS + LAG * (ROWS - 1)] * 2
    assert [c.encode_progress() for c in ctxs] == [14, 7]                # each rank coded exactly its rows
    want_ss = alone(RAGGED_SEED)["ss"]
    for k in range(2):
        cost, bits, dist, parts, nc = out[k]
        assert np.array_equal(cost, G[KEY16 + "/cost"]) and np.array_equal(bits, G[KEY16 + "/bits"]) and np.array_equal(dist, G[KEY16 + "/dist"]), k
        check_parts_against_golden(G, KEY16, plain(parts))
        check_recon_against_golden(G, KEY16, recon(ctxs[k]))
        for c, s in enumerate(ssref(ctxs[k])):
            assert np.array_equal(s, want_ss[c]), (k, c, np.argwhere(s != want_ss[c])[:5])
    for c in ctxs: c.close()


@pytest.mark.parametrize("key,mi", RAGGED)
def test_decode_with_partial_ctus_equals_encode(key, mi):
    """hop_decode_frame from the lag-5 encoder's syntax, both schedules, the SS reference and the loop filters included"""
    from test_gpu_decode import check_roundtrip
    Y, Cb, Cr = ragged_picture(mi)
    parts = check_roundtrip(W, H, Y, Cb, Cr, mi=mi, lag=LAG, slots=16)
    check_parts_against_golden(ragged_golden(), key, plain(parts))


# ---------------------------------------------------------------- the spine's byte-moving entries ----------------------------------------------------------------

SW, SH = 176, 120                        # 2 CTU columns + 48, 1 CTU row + 56
STASH_SLOTS = 16 * 2048                  # k_spine.hip: 16 per CTU row in flight (hop_spine.h: SPINE_LANES)


def random_planes(rng):
    return [rng.integers(0, 256, (SH, SW)).astype(np.int16), rng.integers(0, 256, (SH // 2, SW // 2)).astype(np.int16), rng.integers(0, 256, (SH // 2, SW // 2)).astype(np.int16)]


def upload(ctx, planes):
    for c in range(3):
        ctx.plane_upload("recon", c, planes[c])


def paste(dst, src, x, y, s, sx=None, sy=None):
    """the block (x, y, s) of the three planes src (taken at sx, sy) into dst"""
    sx, sy = x if sx is None else sx, y if sy is None else sy
    dst[0][y:y + s, x:x + s] = src[0][sy:sy + s, sx:sx + s]
    for c in (1, 2):
        dst[c][y // 2:(y + s) // 2, x // 2:(x + s) // 2] = src[c][sy // 2:(sy + s) // 2, sx // 2:(sx + s) // 2]


def edge_blocks(s):
    """the blocks of size s at the picture's four corners (those that fit): they touch the right and the bottom edge where s divides into them"""
    xr, yb = (SW - s) // s * s, (SH - s) // s * s
    return sorted({(0, 0), (xr, 0), (0, yb), (xr, yb)})


def refused(fn, *a):
    with pytest.raises(hp.HopError) as e:
        fn(*a)
    assert e.value.code == hp.HOP_ERR_ARG, e.value
    return True


@pytest.mark.parametrize("slots", [0, 2])
def test_recon_stash_moves_exactly_the_named_blocks(slots):
    """hop_recon_stash: stash, overwrite, restore -- blocks of every size at the picture's corners, stash slots 0 and 1023 among them; only the named rectangles change, in
    all three planes.  With candidate slots: the same through copy k of the pictures (y + k * pic_h).  Refused blocks change nothing"""
    rng = np.random.default_rng(26)
    ctx = hp.Context(SW, SH, slots=slots)
    for s in (8, 16, 32, 64):
        A, B = random_planes(rng), random_planes(rng)
        blocks = edge_blocks(s)
        ids = [0, 1023, 17, STASH_SLOTS - 1][:len(blocks)]
        upload(ctx, A)
        ctx.recon_stash([(x, y, s, i) for (x, y), i in zip(blocks, ids)])
        assert all(np.array_equal(a, b) for a, b in zip(recon(ctx), A))          # putting aside changes nothing
        upload(ctx, B)
        ctx.recon_stash([(x, y, s, i) for (x, y), i in zip(blocks, ids)], restore=True)
        want = [p.copy() for p in B]
        for x, y in blocks: paste(want, A, x, y, s)
        got = recon(ctx)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (s, c, np.argwhere(got[c] != want[c])[:5])
        # a slot keeps its block until it is written again: block 0 once more, somewhere else of the same size
        x0, y0 = blocks[0]; x1, y1 = blocks[-1]
        ctx.recon_stash([(x1, y1, s, ids[0])], restore=True)
        paste(want, A, x1, y1, s, x0, y0)
        got = recon(ctx)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (s, c)
        for k in range(1, slots + 1):                                            # through copy k: out of copy 0 into the copy, copy 0 rewritten, back again
            into = [(x, y + k * SH, s, i) for (x, y), i in zip(blocks, ids)]
            upload(ctx, A)
            ctx.recon_stash([(x, y, s, i) for (x, y), i in zip(blocks, ids)])
            ctx.recon_stash(into, restore=True)
            assert all(np.array_equal(a, b) for a, b in zip(recon(ctx), A)), (s, k)   # copy 0 untouched by the copy's blocks
            upload(ctx, B)
            ctx.recon_stash([(x, y, s, 100 + j) for j, (x, y, _, _) in enumerate(into)])
            ctx.recon_stash([(x, y, s, 100 + j) for j, (x, y) in enumerate(blocks)], restore=True)
            want = [p.copy() for p in B]
            for x, y in blocks: paste(want, A, x, y, s)
            got = recon(ctx)
            for c in range(3):
                assert np.array_equal(got[c], want[c]), (s, k, c, np.argwhere(got[c] != want[c])[:5])
    # refusals: nothing is enqueued, the picture stays
    P = random_planes(rng)
    upload(ctx, P)
    bad = [(128, 0, 64, 0),                        # crosses the right edge (128 + 64 > 176)
           (0, 64, 64, 0), (0, 96, 32, 0),         # cross the bottom edge (120)
           (168, 112, 16, 0),                      # misaligned for its size, and across both edges
           (4, 0, 8, 0), (0, 4, 8, 0), (8, 0, 16, 0), (0, 16, 32, 0),   # misaligned
           (0, 0, 12, 0), (0, 0, 4, 0), (0, 0, 128, 0), (0, 0, 0, 0),   # not a CU size
           (-8, 0, 8, 0), (0, -8, 8, 0),
           (0, 0, 8, -1), (0, 0, 8, STASH_SLOTS), (0, 0, 8, 1 << 30),   # no such stash slot
           (0, (slots + 1) * SH, 8, 0),            # no such copy
           (0, slots * SH + 96, 32, 0)]            # out of the bottom of the last copy
    for b in bad:
        for restore in (False, True):
            assert refused(ctx.recon_stash, [b], restore), b
            assert refused(ctx.recon_stash, [(0, 0, 8, 5), b], restore), b           # one bad block refuses the call
    assert all(np.array_equal(a, b) for a, b in zip(recon(ctx), P))
    ctx.close()


def commit_reference(planes, blocks):
    """the oracle's restatement of xCopyYuv2SSRef on sentinel planes: the blocks' samples, then ONE commit (its last block), which re-extends all borders"""
    O = oracle()
    pl = Planes(SW, SH)
    for x, y, s in blocks:
        pl.y00()[y:y + s, x:x + s] = planes[0][y:y + s, x:x + s]
        pl.bufCb[40 + y // 2:40 + (y + s) // 2, 40 + x // 2:40 + (x + s) // 2] = planes[1][y // 2:(y + s) // 2, x // 2:(x + s) // 2]
        pl.bufCr[40 + y // 2:40 + (y + s) // 2, 40 + x // 2:40 + (x + s) // 2] = planes[2][y // 2:(y + s) // 2, x // 2:(x + s) // 2]
    x, y, s = blocks[-1]
    by, bb, br = (np.ascontiguousarray(planes[0][y:y + s, x:x + s]), np.ascontiguousarray(planes[1][y // 2:(y + s) // 2, x // 2:(x + s) // 2]),
                  np.ascontiguousarray(planes[2][y // 2:(y + s) // 2, x // 2:(x + s) // 2]))
    O.hop_o_ssref_commit_cu(pl.ptr00(0), pl.ptr00(1), pl.ptr00(2), SW, SH, x, y, s, p16(by), p16(bb), p16(br))
    return pl


def causal_blocks(last_rows=7):
    """coding order: the full CTUs of row 0 as 64x64 blocks, the 48-wide one as 8x8 blocks, then the 56-tall row's first CTU and the 48x56 corner CTU as 8x8 blocks; the
    CTU between those two is left out (last_rows < 7: only that many 8-sample rows of the corner CTU)"""
    b = [(0, 0, 64), (64, 0, 64)] + [(x, y, 8) for y in range(0, 64, 8) for x in range(128, SW, 8)]
    b += [(x, y, 8) for y in range(64, SH, 8) for x in range(0, 64, 8)]
    b += [(x, y, 8) for y in range(64, 64 + 8 * last_rows, 8) for x in range(128, SW, 8)]
    return b


@pytest.mark.parametrize("slots", [0, 2])
def test_ssref_commit_recon_of_partial_ctus_equals_the_oracle(slots):
    """hop_ssref_commit_recon from the resident reconstruction: the partial CTUs on the right, below and in the corner as 8x8 blocks (what import_block commits for a block
    of another rank), one call per CTU in coding order -- against the oracle's commit, margins included; what was not committed is still the sentinel"""
    rng = np.random.default_rng(27)
    P = random_planes(rng)
    ctx = hp.Context(SW, SH, slots=slots)
    ctx.ssref_reset()
    upload(ctx, P)
    blocks = causal_blocks()
    done = []
    for lo, hi in ((0, 1), (1, 2), (2, 2 + 48), (2 + 48, 2 + 48 + 56), (2 + 48 + 56, len(blocks))):
        ctx.ssref_commit_recon(blocks[lo:hi])
        done += blocks[lo:hi]
        pl = commit_reference(P, done)
        for c, want in enumerate((pl.bufY, pl.bufCb, pl.bufCr)):
            got = ctx.ssref_download(c)
            assert np.array_equal(got, want), (hi, c, np.argwhere(got != want)[:5])
    got = ctx.ssref_download(0)
    assert np.all(got[M + 64:M + SH, M + 64:M + 128] == -1) and np.all(got[M + SH:, M + 64:M + 128] == -1)      # the CTU never committed, and the margin below it
    assert np.all(got[M + SH:, M + 128:] == got[M + SH - 1, M + 128:]) and got[M + SH - 1, M + SW - 1] == P[0][SH - 1, SW - 1]
    before = ssref(ctx)
    for b in [(128, 64, 64), (160, 96, 32), (0, 112, 16), (4, 0, 8), (0, 0, 12), (-8, 0, 8), (SW, 0, 8), (0, SH, 8)]:
        assert refused(ctx.ssref_commit_recon, [b]), b
        assert refused(ctx.ssref_commit_recon, [(0, 0, 8), b]), b
    assert all(np.array_equal(a, b) for a, b in zip(before, ssref(ctx)))
    ctx.close()


def test_valid_pattern_answers_from_the_resident_ss_reference():
    """hop_valid_pattern: a few hundred queries over a half-committed picture (bottom row: the first CTU whole, the next one not at all, the corner CTU down to row 87)
    answered from the downloaded plane in numpy; probes on the first sentinel row below the committed rows, in the margins, and refusals for probes outside the padded plane"""
    rng = np.random.default_rng(28)
    P = random_planes(rng)
    ctx = hp.Context(SW, SH)
    ctx.ssref_reset()
    upload(ctx, P)
    ctx.ssref_commit_recon(causal_blocks(last_rows=3))
    ss = ctx.ssref_download(0).astype(np.int32)
    q = []
    for _ in range(400):
        w, h = (int(v) for v in rng.choice([4, 8, 12, 16, 24, 32, 64], 2))
        x, y = int(rng.integers(0, SW // 4)) * 4, int(rng.integers(0, SH // 4)) * 4
        row, col = int(rng.integers(-M, SH + M)), int(rng.integers(-M, SW + M - w - 4))   # where the probes fall: anywhere in the padded plane
        q.append((x, y, w, h, 4 * (col - x) + int(rng.integers(0, 4)), 4 * (row - h - 4 - y) + int(rng.integers(0, 4))))
    edge = len(q)
    for x, w in ((0, 8), (40, 16), (128, 16), (128 + 16, 16), (SW - 8, 4), (56, 8)):
        for row in (87, 88, SH - 1, SH, SH + M - 1):                             # the corner CTU's last committed row, the first sentinel row below it, the picture's last row, the margin below it
            q.append((x, row - 8 - 4, w, 8, 0, 0))
    for row in (-M, -1, 0, 63, 64):                                              # left, right and top margins
        q += [(0, 0, 8, 8, 4 * -M, 4 * (row - 12)), (0, 0, 8, 8, 4 * (SW + M - 13), 4 * (row - 12)), (64, 0, 8, 8, 4 * -8 + 3, 4 * (row - 12) + 1)]
    q = np.array(q, np.int32)
    row = q[:, 1] + (q[:, 5] >> 2) + q[:, 3] + 4
    col = q[:, 0] + (q[:, 4] >> 2)
    assert row.min() >= -M and row.max() < SH + M and col.min() >= -M and (col + q[:, 2] + 4).max() < SW + M
    want = ((ss[M + row, M + col] != -1) & (ss[M + row, M + col + q[:, 2] + 4] != -1)).astype(np.uint8)
    got = ctx.valid_pattern(q)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert 0.1 < want.mean() < 0.9                                               # both answers are well represented
    # under the first CTU everything down to the last margin row is committed; under the corner CTU (its right margin included: the probe at column 176) row 88 and all
    # below it are the sentinel; a probe in the CTU that was left out fails everywhere
    assert want[edge:edge + 30].reshape(6, 5).tolist() == [[1] * 5, [1] * 5, [1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0] * 5]
    assert want[edge + 30:].reshape(5, 3).tolist() == [[1, 1, 1]] * 4 + [[1, 1, 0]]   # margins left, right and (vector -29 / 4 -> -8 samples) a probe that lands in the CTU left out from row 64 on
    G = 64                                                                       # guard rows above and below the padded plane: probes there are allowed, beyond them refused
    for b in [(0, 0, 8, 8, 4 * (-M - 1), 0), (0, 0, 8, 8, 4 * (SW + M - 12), 0), (0, 0, 8, 8, 0, 4 * (-M - G - 1 - 12)), (0, 0, 8, 8, 0, 4 * (SH + M + G - 12)),
              (SW - 8, 0, 8, 8, 4 * M, 0)]:
        assert refused(ctx.valid_pattern, [b]), b
        assert refused(ctx.valid_pattern, [q[0], b]), b
    assert ctx.valid_pattern(np.zeros((0, 6), np.int32)).size == 0
    ctx.close()


def zidx(x4, y4):
    z = 0
    for b in range(4):
        z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1))
    return z


@pytest.mark.parametrize("slots", [0, 2])
def test_recon_and_coef_put_device_write_exactly_their_cus(slots):
    """hop_recon_put_device + hop_coef_put_device: packed CUs of 8, 16 and 64 samples at the picture's edges into the reconstruction picture and the image of the levels
    (which a small encode creates first); then, since the levels now exist, hop_recon_stash carries them with the samples -- also through the candidate slots' copies"""
    import torch
    rng = np.random.default_rng(29)
    Y, Cb, Cr = lenslet(SW, SH, 16, 9)
    ctx = hp.Context(SW, SH, slots=slots)
    ctx.upload_orig(Y, Cb, Cr)
    ctx.encode_frame(32, 16)                                                     # (raster order, 6 CTUs: leaves a reconstruction and the levels' image)
    rec, lv = recon(ctx), ctx.levels_download()
    wctu = (SW + 63) // 64
    assert lv.shape == (6, 6144) and np.abs(lv).sum() > 0

    def put(cus, s, copy=0, residual=True):
        """-> the packed planes and levels it sent"""
        n, l2 = len(cus), s.bit_length() - 1
        jobs = np.zeros(n, hp.RQT_JOB_DTYPE)
        jobs["x"], jobs["y"], jobs["log2_cu"] = [c[0] for c in cus], [c[1] + copy * SH for c in cus], l2
        ry = rng.integers(0, 256, (n, s, s)).astype(np.int16); rc = rng.integers(0, 256, (n, 2, s // 2, s // 2)).astype(np.int16)
        co = rng.integers(-300, 300, (n, s * s * 3 // 2)).astype(np.int32)
        d = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in (jobs, ry, rc, co)]
        torch.cuda.synchronize()
        ctx.recon_put_device(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr())
        ctx.coef_put_device(n, d[0].data_ptr(), d[3].data_ptr() if residual else None)
        ctx.sync()
        return ry, rc, co if residual else np.zeros_like(co)

    def expect(rec, lv, cus, s, ry, rc, co):
        for i, (x, y) in enumerate(cus):
            rec[0][y:y + s, x:x + s] = ry[i]
            for c in (1, 2): rec[c][y // 2:(y + s) // 2, x // 2:(x + s) // 2] = rc[i, c - 1]
            a, z = (y >> 6) * wctu + (x >> 6), zidx((x & 63) >> 2, (y & 63) >> 2)
            lv[a, 16 * z:16 * z + s * s] = co[i, :s * s]
            lv[a, 4096 + 4 * z:4096 + 4 * z + s * s // 4] = co[i, s * s:s * s * 5 // 4]
            lv[a, 5120 + 4 * z:5120 + 4 * z + s * s // 4] = co[i, s * s * 5 // 4:]

    def check(what):
        got = recon(ctx)
        for c in range(3):
            assert np.array_equal(got[c], rec[c]), (what, c, np.argwhere(got[c] != rec[c])[:5])
        g = ctx.levels_download()
        assert np.array_equal(g, lv), (what, np.argwhere(g != lv)[:5])

    cases = [(8, [(SW - 8, SH - 8), (SW - 8, 0), (0, SH - 8), (64, 56), (128, 64), (120, 112)]), (16, [(160, 96), (160, 0), (0, 96), (112, 48)]), (64, [(64, 0), (0, 0)])]
    for s, cus in cases:
        expect(rec, lv, cus, s, *put(cus, s))
        check(("put", s))
    cus = [(SW - 8, SH - 8), (128, 64)]
    expect(rec, lv, cus, 8, *put(cus, 8, residual=False))                        # CUs without residual: their levels are cleared
    check("no residual")
    for k in range(1, slots + 1):                                                # into copy k: copy 0 keeps its samples and levels; brought over by the stash, levels with them
        for s, cus in cases[:2]:
            sent = put(cus, s, copy=k)
            check(("copy untouched", k, s))
            ctx.recon_stash([(x, y + k * SH, s, 40 + i) for i, (x, y) in enumerate(cus)])
            ctx.recon_stash([(x, y, s, 40 + i) for i, (x, y) in enumerate(cus)], restore=True)
            expect(rec, lv, cus, s, *sent)
            check(("copy", k, s))
    ctx.close()
