"""GPU: the two forms of the fractional and the GT search.  A request of up to HOP_ME_WIDE_MAX PUs runs k_frac and k_gt_search as ONE launch each, a workgroup of several
waves per PU indexed directly (the small-batch form); a larger one sorts its PUs into two size classes (k_gt_prep) and runs one wave per PU of at most 16x16 and four per
larger PU (the large-batch form, what every request ran before).  Nothing a PU computes depends on how many waves share its items, so both forms must write the same
bytes: here every batch goes through hop_me_search with HOP_ME_WIDE=0 (always the large-batch form) and HOP_ME_WIDE=2 (always the small-batch form), every field of
every result row is compared, and both are compared with the restatement (hop_o_me_pu) the way tests/test_gpu_parity.py::test_me_random_vs_oracle_10bit_and_sad does.
With the switch unset the other GPU modules' small requests take the small-batch form; this module is what keeps the large-batch form covered at small sizes.

About the start vectors of the GT search: start 0 is the best integer vector, and a PU whose best integer vector is (0,0) is not valid (TEncSearch.cpp:4603-4606), so
its fractional and GT searches do not run at all -- "start 0 skipped" and "every start skipped" exist only as such PUs.  They are in the batches (ZERO_WINDOW below),
next to PUs with an empty window, both in the middle of a batch: their rows must come back as the SS search left them, in both forms."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import degenerate as dg
from hoputil import ROOT, Planes, lambda_for_qp, lenslet, oracle, p16

pytestmark = pytest.mark.gpu

HOP_ME_WIDE_MAX = 512           # hevc-hop_amd/csrc/k_gt_search.hip: requests of up to this many PUs take the small-batch form when HOP_ME_WIDE is unset
W, H = 256, 192
# the shapes of test_me_random_vs_oracle_10bit_and_sad and the 4-multiple sides that take the 4x4 Hadamard path
SHAPES = [(64, 64), (32, 32), (16, 16), (8, 8), (64, 32), (16, 32), (48, 64), (32, 24), (8, 4), (4, 8), (12, 16), (16, 4), (64, 16), (16, 64), (32, 8), (8, 32)]


def _hophip():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def hp():
    return _hophip()


def _res_row(r):
    """hop_pu_result -> the 27-entry layout of oracle/ref_harness.cpp:ref_me_pu"""
    return ([int(r["mv_int"][0]), int(r["mv_int"][1]), int(r["sad"]), int(r["not_valid"])] + [int(v) for v in r["half"]] +
            [int(v) for v in r["qter"]] + [int(r["frac_cost"]), int(r["gt_flag"])] + [int(v) for v in r["gt"]] +
            [int(r["cost"])] + [int(v) for v in r["mv_final"]] + [int(v) for v in r["half_final"]] + [int(v) for v in r["qter_final"]] +
            [int(r["mv_int"][0]), int(r["mv_int"][1])])


def _planes(Y):
    """the SS reference of test_me_random_vs_oracle_10bit_and_sad: two CTU rows and half of the third coded, a hole of sentinels inside, the border extended"""
    pl = Planes(W, H)
    pl.y00()[:128, :W] = Y[:128]
    pl.y00()[128:192, :128] = Y[128:192, :128]
    pl.y00()[40:52, 60:90] = -1
    by = np.ascontiguousarray(pl.y00()[0:8, 0:8]); z = np.zeros((4, 4), np.int16) - 1
    oracle().hop_o_ssref_commit_cu(pl.ptr00(0), pl.ptr00(1), pl.ptr00(2), W, H, 0, 0, 8, p16(by), p16(z), p16(z))
    return pl


def _jobs(hp, seed, lc, flags):
    """two PUs of every shape (the first inside the uncoded CTU at (128,128), the second in the third CTU row's coded part or at the picture's left edge), n_amvp 0, 1, 2 in
    turn, zero AMVP vectors (a skipped start) among them; then, in the middle of the batch, the PUs that are not valid"""
    O = oracle()
    rng = np.random.default_rng(seed)
    jobs = np.zeros(2 * len(SHAPES) + 6, hp.PU_JOB_DTYPE)
    special = {9: "empty", 10: "zero", 20: "empty", 21: "zero", 22: "empty", 30: "zero"}         # rows of the batch that get a PU that is not valid
    k = 0
    for i in range(len(jobs)):
        j = jobs[i]
        if i in special:
            w, h = SHAPES[(3 * i) % len(SHAPES)]
            j["pu_x"], j["pu_y"], j["w"], j["h"] = 64, 64, w, h
            if special[i] == "empty":                                   # rng_right < rng_left: no candidate at all
                j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"] = 0, -1, 0, -1
            else:                                                       # ZERO_WINDOW: the window holds the PU's own (coded) position and the predictor is (0,0): the best
                j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"] = -4, 4, -4, 4      # integer vector is (0,0) at SAD 0
            j["lambda_cost"], j["n_amvp"], j["amvp"], j["flags"] = lc, 2, [8, -64, 0, 0], flags
            continue
        w, h = SHAPES[k % len(SHAPES)]
        cuS = 64 if max(w, h) > 32 else 32 if max(w, h) > 16 else 16 if max(w, h) > 8 else 8
        cuX, cuY = (128, 128) if k < len(SHAPES) else (int(rng.integers(0, 2)) * 64, 128)
        puX, puY = cuX + (cuS - w) * (k & 1), cuY + (cuS - h) * (k & 1)
        pred = (int(rng.integers(-50, 50)), int(rng.integers(-200, -30)))
        o6 = (ctypes.c_int * 6)()
        O.hop_o_set_search_range(W, H, cuX, cuY, cuS, 2 * 4 + cuX // 64, 4, pred[0], pred[1], 128, puX - cuX, puY - cuY, 0, int(cuX == 0), o6)
        j["pu_x"], j["pu_y"], j["w"], j["h"] = puX, puY, w, h
        j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"], j["off_x"], j["off_y"] = list(o6)
        j["pred_x"], j["pred_y"], j["lambda_cost"], j["n_amvp"] = pred[0], pred[1], lc, (k + k // len(SHAPES)) % 3
        a = [pred[0], pred[1], int(rng.integers(-40, 40)), int(rng.integers(-300, -60))]
        if k % 5 == 1: a[0:2] = [0, 0]                                  # a zero AMVP vector: that start is skipped
        if k % 7 == 3: a[2:4] = [0, 0]
        if k % 11 == 5: a = [0, 0, 0, 0]                                # only start 0 is left
        j["amvp"] = a
        j["flags"] = flags
        k += 1
    return jobs


def _oracle_rows(hp, jobs, Y, pl, lc, flags, bd):
    O = oracle()
    rows = []
    for j in jobs:
        out = (ctypes.c_int64 * 32)()
        org = np.ascontiguousarray(Y[j["pu_y"]:j["pu_y"] + j["h"], j["pu_x"]:j["pu_x"] + j["w"]])
        O.hop_o_me_pu(p16(org), int(j["w"]), pl.ptr00(0), pl.sy, int(j["pu_x"]), int(j["pu_y"]), int(j["w"]), int(j["h"]),
                      int(j["rng_left"]), int(j["rng_right"]), int(j["rng_top"]), int(j["rng_bottom"]), int(j["off_x"]), int(j["off_y"]),
                      int(j["pred_x"]), int(j["pred_y"]), int(j["n_amvp"]), (ctypes.c_int * 4)(*[int(v) for v in j["amvp"]]), lc,
                      1 if flags & hp.HOP_FLAG_FEN else 0, 1 if flags & hp.HOP_FLAG_HADME else 0, bd, 3, out)
        rows.append(list(out)[:27])
    return rows


def _search(ctx, jobs, switch, monkeypatch):
    """hop_me_search to the GT stage with HOP_ME_WIDE = switch (None: unset); the library reads it on every call"""
    with monkeypatch.context() as m:
        if switch is None: m.delenv("HOP_ME_WIDE", raising=False)
        else: m.setenv("HOP_ME_WIDE", switch)
        return ctx.me_search(jobs, 3)


def _check_batch(ctx, jobs, want, monkeypatch, where):
    """both forms: the same bytes, and the restatement's results"""
    classes = _search(ctx, jobs, "0", monkeypatch)
    wide = _search(ctx, jobs, "2", monkeypatch)
    for i, (j, a, b, w) in enumerate(zip(jobs, classes, wide, want)):
        tag = (where, i, [int(j[k]) for k in ("pu_x", "pu_y", "w", "h", "n_amvp")], [int(v) for v in j["amvp"]])
        for f in a.dtype.names:
            assert np.array_equal(a[f], b[f]), (tag, f, a[f], b[f])
        got = _res_row(b)
        if w[3]:
            assert got[2:4] == w[2:4], (tag, got, w)
        else:
            assert got[:25] == w[:25], (tag, got, w)
    assert classes.tobytes() == wide.tobytes(), where


def _split(jobs):
    large = np.array([max(int(j["w"]), int(j["h"])) > 16 for j in jobs])
    return large


@functools.lru_cache(maxsize=None)
def _content(bd):
    return lenslet(W, H, 14, 31 + bd, bitdepth=bd)


@pytest.mark.parametrize("fen", [1, 0])
@pytest.mark.parametrize("hadme", [1, 0])
@pytest.mark.parametrize("bd", [8, 10])
def test_both_forms_write_the_same_bytes(hp, bd, hadme, fen, monkeypatch):
    """lenslet content, 8 and 10 bit, HadamardME and FEN on and off: the mixed batch, its large PUs alone, its small PUs alone (each with the PUs that are not valid kept in
    the middle) and single PUs -- a large one, a small one, a 4x4-Hadamard one and one that is not valid"""
    flags = (hp.HOP_FLAG_FEN if fen else 0) | (hp.HOP_FLAG_HADME if hadme else 0)
    Y, Cb, Cr = _content(bd)
    pl = _planes(Y)
    lam, lc = lambda_for_qp(27 + 3 * fen + hadme)
    jobs = _jobs(hp, 100 + bd + flags, lc, flags)
    want = _oracle_rows(hp, jobs, Y, pl, lc, flags, bd)
    n_bad = sum(1 for w in want if w[3])
    assert n_bad >= 6 and len(jobs) - n_bad >= 24, n_bad          # the six made PUs are not valid and most of the others are
    ctx = hp.Context(W, H, bit_depth=bd)
    ctx.upload_orig(Y, Cb, Cr)
    ctx.ssref_upload(0, pl.bufY)
    large = _split(jobs)
    bad = np.array([bool(w[3]) for w in want])
    _check_batch(ctx, jobs, want, monkeypatch, "mixed")
    for name, sel in (("large", large | bad), ("small", ~large | bad)):
        idx = np.nonzero(sel)[0]
        _check_batch(ctx, jobs[idx], [want[i] for i in idx], monkeypatch, name)
    for i in (0, 3, 8, 9, 10, 14):                                # (64,64), (8,8), (8,4), empty window, best vector (0,0), (64,16) after the shift by the made PUs
        _check_batch(ctx, jobs[i:i + 1], want[i:i + 1], monkeypatch, "single %d" % i)
    ctx.close()


def test_threshold_unset_switch(hp, monkeypatch):
    """the switch unset: a batch of HOP_ME_WIDE_MAX - 1 and of HOP_ME_WIDE_MAX PUs (the small-batch form) and one of HOP_ME_WIDE_MAX + 1 (the large-batch form), each
    the bytes of HOP_ME_WIDE=0"""
    flags = hp.HOP_FLAG_FEN | hp.HOP_FLAG_HADME
    Y, Cb, Cr = _content(8)
    pl = _planes(Y)
    lam, lc = lambda_for_qp(30)
    base = _jobs(hp, 7, lc, flags)
    ctx = hp.Context(W, H)
    ctx.upload_orig(Y, Cb, Cr)
    ctx.ssref_upload(0, pl.bufY)
    for n in (HOP_ME_WIDE_MAX - 1, HOP_ME_WIDE_MAX, HOP_ME_WIDE_MAX + 1):
        jobs = np.ascontiguousarray(np.resize(base, n))
        ref = _search(ctx, jobs, "0", monkeypatch)
        got = _search(ctx, jobs, None, monkeypatch)
        assert got.tobytes() == ref.tobytes(), n
        assert int((ref["not_valid"] == 0).sum()) > n // 2, n
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", ["flat_mid", "tile8"])
def test_both_forms_on_tied_content(hp, name, bd, monkeypatch):
    """a flat and an exactly 8-periodic picture (tests/degenerate.py): every candidate ties, first-best in visit order is the whole result"""
    flags = hp.HOP_FLAG_FEN | hp.HOP_FLAG_HADME
    Y, Cb, Cr = dg.picture(name, W, H, bd)
    pl = _planes(Y)
    lam, lc = lambda_for_qp(32)
    jobs = _jobs(hp, 900 + bd, lc, flags)
    want = _oracle_rows(hp, jobs, Y, pl, lc, flags, bd)
    assert sum(1 for w in want if not w[3]) >= 16
    ctx = hp.Context(W, H, bit_depth=bd)
    ctx.upload_orig(Y, Cb, Cr)
    ctx.ssref_upload(0, pl.bufY)
    _check_batch(ctx, jobs, want, monkeypatch, name)
    ctx.close()
