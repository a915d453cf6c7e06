"""CPU: the restatement and the RD spine over it on degenerate pictures (tests/degenerate.py: flat, exactly periodic, two-level, clipped) against what the REFERENCE's own
code did on them (tests/golden/degenerate.npz, oracle/make_golden25.py).  On this content many candidates of a search cost exactly the same, so the reference's first-best
rule (strict `<` in its visit order) decides, and the clips of the interpolation filters, the GT warp and the intra edge filters are reached.

The module also states, on what the golden RECORDED (not on anything a kernel computes), the shares of ties and clips that keep tests/test_gpu_degenerate.py from passing
vacuously."""
import ctypes

import numpy as np
import pytest

import degenerate as dg
from goldutil import coded_planes, crc, load
from hoputil import oracle, p16
from test_spine_cpu import check_against_golden, run_cpu, run_cpu_wpp, spine_cpu

VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def G():
    return load("degenerate.npz")


def me_scenarios(G, name):
    """Yields (planes, Y, Cb, Cr, jobs, outs, tied, lambda_cost) per coded-area scenario of me/<name> (the layout of me_chain.npz, goldutil.me_chain_scenarios)"""
    Y, Cb, Cr = dg.picture(name, dg.ME_W, dg.ME_H)
    assert dg.pic_crc((Y, Cb, Cr)) == int(G["me/%s/pic_crc" % name])
    jobs, outs, tied = G["me/%s/jobs" % name], G["me/%s/outs" % name], G["me/%s/tied" % name]
    pi = 0
    for si, (cr_, cc_, npart) in enumerate(G["me/scen"]):
        part = [tuple(int(v) for v in G["me/partial"][pi + k]) for k in range(npart)]
        pi += npart
        pl = coded_planes(Y, Cb, Cr, dg.ME_W, dg.ME_H, int(cr_), int(cc_), part)
        assert [crc(pl.bufY), crc(pl.bufCb), crc(pl.bufCr)] == [int(v) for v in G["me/%s/planes_crc" % name][si]]
        sel = jobs[:, 0] == si
        yield pl, Y, Cb, Cr, jobs[sel], outs[sel], tied[sel], int(G["me/lambda_cost"])


def pred_case(G, name):
    """planes, jobs, expected outputs per job of pred/<name>"""
    Y, Cb, Cr = dg.picture(name, dg.ME_W, dg.ME_H)
    assert dg.pic_crc((Y, Cb, Cr)) == int(G["pred/%s/pic_crc" % name])
    pl = coded_planes(Y, Cb, Cr, dg.ME_W, dg.ME_H, 3, 2, [(128, 192, 32)])
    assert [crc(pl.bufY), crc(pl.bufCb), crc(pl.bufCr)] == [int(v) for v in G["pred/%s/planes_crc" % name]]
    ends = np.cumsum(G["pred/%s/out_len" % name])
    flat = G["pred/%s/out_flat" % name]
    wants = [flat[e - n:e] for e, n in zip(ends, G["pred/%s/out_len" % name])]
    return pl, (Y, Cb, Cr), G["pred/%s/jobs" % name], wants


INTRA_KEYS = ["%s_%s" % (n, s) for n in dg.INTRA_RECS for s in ("same", "inv")]


def intra_case(G, key):
    """reconstruction, original, jobs (x, y, N, strong), neighbour flags, the 35 SATDs per block of intra/<key>"""
    name, side = key.rsplit("_", 1)
    rec = np.ascontiguousarray(dg.picture(name, dg.INTRA_W, dg.INTRA_H)[0])
    assert crc(rec) == int(G["intra/%s/rec_crc" % key])
    org = np.ascontiguousarray(255 - rec if side == "inv" else rec)
    return rec, org, G["intra/%s/jobs" % key], G["intra/%s/flags" % key], G["intra/%s/satd" % key]


# ---- the restatement against the golden ----
@pytest.mark.parametrize("name", dg.ME_PICTURES)
def test_me_pu_on_degenerate_pictures(G, name):
    O = oracle()
    n = 0
    for pl, Y, _, _, jobs, outs, _, lc in me_scenarios(G, name):
        for job, want in zip(jobs, outs):
            (_, puX, puY, w, h, cuX, cuY, cuS, offx, offy, fr, fc, px, py, l, r, t, b, ox, oy, nA) = [int(v) for v in job[:21]]
            o6 = (ctypes.c_int * 6)()
            O.hop_o_set_search_range(pl.W, pl.H, cuX, cuY, cuS, (cuY // 64) * 5 + cuX // 64, 5, px, py, 128, offx, offy, fr, fc, o6)
            assert list(o6) == [l, r, t, b, ox, oy]
            org = np.ascontiguousarray(Y[puY:puY + h, puX:puX + w])
            out = (ctypes.c_int64 * 32)()
            O.hop_o_me_pu(p16(org), w, pl.ptr00(0), pl.sy, puX, puY, w, h, l, r, t, b, ox, oy, px, py, nA, (ctypes.c_int * 4)(*[int(v) for v in job[21:25]]), lc, 1, 1, 8, 3, out)
            got, want = list(out)[:27], [int(v) for v in want]
            if want[3]:        # not valid: only the integer stage is defined
                assert got[2:4] == want[2:4], (name, job)
            else:
                assert got[:25] == want[:25], (name, job, got, want)
            n += 1
    assert n == 32           # no PU is left out of the comparison


@pytest.mark.parametrize("name", dg.PRED_PICTURES)
def test_pred_inter_on_degenerate_pictures(G, name):
    O = oracle()
    pl, _, jobs, wants = pred_case(G, name)
    for job, want in zip(jobs, wants):
        puX, puY, w, h, mvx, mvy, useGT = [int(v) for v in job[:7]]
        a = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        O.hop_o_pred_inter(pl.ptr00(0), pl.sy, pl.ptr00(1), pl.ptr00(2), pl.sc, puX, puY, w, h, mvx, mvy, useGT, (ctypes.c_int * 8)(*[int(v) for v in job[7:15]]), 8, 8,
                           p16(a[0]), p16(a[1]), p16(a[2]))
        assert np.array_equal(np.concatenate([x.ravel() for x in a]), want), (name, [int(v) for v in job])
    assert len(jobs) == 48


@pytest.mark.parametrize("key", INTRA_KEYS)
def test_intra_rough_on_degenerate_pictures(G, key):
    O = oracle()
    rec, org, jobs, flags, satd = intra_case(G, key)
    for (x, y, N, strong), fl, want in zip(jobs, flags, satd):
        s = (ctypes.c_uint32 * 35)()
        fl = np.ascontiguousarray(fl)
        O.hop_o_intra_rough(p16(rec), dg.INTRA_W, p16(org), dg.INTRA_W, int(x), int(y), int(N), fl.ctypes.data_as(VP), 8, int(strong), s)
        assert list(s) == [int(v) for v in want], (key, int(x), int(y), int(N))
    assert len(jobs) == 30


@pytest.mark.parametrize("key,name,W,H,wpp", dg.SPINE_FRAMES)
def test_spine_on_degenerate_pictures(G, key, name, W, H, wpp):
    """every candidate of xCheckBestMode, per-CTU cost / bits / distortion and the finished partition data of the reference encoder; the wavefront picture serially (lag 0)
    and as a wavefront of rows (lag 5)"""
    L = spine_cpu()
    pic = dg.picture(name, W, H)
    assert dg.pic_crc(pic) == int(G["spine/%s/pic_crc" % key])
    S = spine_view(G)
    if not wpp:
        cost, bits, dist, parts, rec, text = run_cpu(L, W, H, *pic)
        check_against_golden(S, key, cost, bits, dist, parts, text)
        return
    for lag in (0, 5):
        cost, bits, dist, parts, rec, text, rr = run_cpu_wpp(L, W, H, *pic, lag)
        check_against_golden(S, key, cost, bits, dist, parts, text)


class _SpineView:
    """degenerate.npz's spine/<key>/... members under the names check_against_golden asks encoder_spine.npz for"""

    def __init__(self, G):
        self.G = G

    def __getitem__(self, k):
        return self.G["spine/" + k]


def spine_view(G):
    return _SpineView(G)


# ---- what the golden must hold for the GPU tests to mean something: asserted on what the reference recorded ----
def test_the_me_set_holds_ties_gt_wins_and_fractional_vectors(G):
    outs = np.concatenate([G["me/%s/outs" % n] for n in dg.ME_PICTURES])
    tied = {n: int(G["me/%s/tied" % n].sum()) for n in dg.ME_PICTURES}
    valid = outs[:, 3] == 0
    n = len(outs)
    print("tied integer-search minimum per picture:", tied, "of 32 each; not valid:", int((~valid).sum()), "of", n, "; GT wins:", int(outs[valid][:, 9].sum()),
          "; non-zero half / quarter vector:", int((valid & (np.abs(outs[:, 21:25]).sum(1) > 0)).sum()))
    assert n == 32 * len(dg.ME_PICTURES) == 224
    assert int((~valid).sum()) * 10 <= n                                              # at most 10 % not valid
    assert sum(tied.values()) * 10 >= n * 6 and min(tied.values()) >= 10             # ties: 60 % of all PUs, 10 of 32 in every picture
    assert int(outs[valid][:, 9].sum()) >= 16                                         # GT wins
    assert int((valid & (np.abs(outs[:, 21:25]).sum(1) > 0)).sum()) >= 40            # a non-zero half or quarter vector


def test_the_predictor_set_reaches_both_ends_of_the_range(G):
    top = zero = 0
    for name in dg.PRED_PICTURES:
        ends = np.cumsum(G["pred/%s/out_len" % name])
        for job, e, n in zip(G["pred/%s/jobs" % name], ends, G["pred/%s/out_len" % name]):
            luma = G["pred/%s/out_flat" % name][e - n:e - n + int(job[2]) * int(job[3])]
            top += int((luma == 255).any()); zero += int((luma == 0).any())
    print("predictor jobs whose luma output holds top:", top, "and 0:", zero, "of", 48 * len(dg.PRED_PICTURES))
    assert top >= 100 and zero >= 100


def test_the_intra_set_holds_equal_satds(G):
    eq = {k: int(sum(len(set(int(v) for v in s)) < 35 for s in G["intra/%s/satd" % k])) for k in INTRA_KEYS}
    n = 30 * len(INTRA_KEYS)
    print("blocks with two modes of equal SATD:", eq, "total", sum(eq.values()), "of", n)
    assert sum(eq.values()) * 10 >= n * 8
