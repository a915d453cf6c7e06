"""CPU: hop_me_reach_above -- the CTU column of the row above that a row of the exact wavefront (hop_encode_set_exact) waits for before a motion search -- against the
formula restated in numpy.  A wait that is too short silently breaks exactness, so the arithmetic is a function of its own; tests/test_gpu_exact_wavefront.py shows on
the device that hop_me_search reads nothing of the row above beyond the column it names."""
import ctypes
import os
import sys

import numpy as np

from hoputil import ROOT

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

BOUND_W, BOUND_H = 448, 192


def bound_jobs(lam=1000):
    """a dozen PUs of CTU row 1 of a 448x192 picture spread over its width, whose windows lie in row 0 (predictors point up, beyond the block's height), with a second AMVP vector that points further to the
    right than the window reaches, or nowhere (0, 0: not a start vector)"""
    jobs = np.zeros(12, hp.PU_JOB_DTYPE)
    shapes = [(64, 64), (32, 64), (64, 16), (16, 16), (8, 4), (32, 32), (16, 8), (8, 8), (64, 32), (16, 32), (32, 16), (4, 8)]
    for i, (w, h) in enumerate(shapes):
        j = jobs[i]
        x, y = 4 * ((29 * i) % 88), 64 + 4 * ((5 * i) % ((64 - h) // 4 + 1))
        px, py = 6 * (i % 5) - 8, -(h + 44 + 2 * (i % 9))                 # the predictor, in samples: the displaced block ends above row 64
        j["pu_x"], j["pu_y"], j["w"], j["h"] = x, y, w, h
        j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"] = px - 12, px + 12, py - 8, py + 8
        j["off_x"], j["off_y"] = 1000, 1000
        j["pred_x"], j["pred_y"], j["lambda_cost"], j["flags"] = 4 * px, 4 * py, lam, hp.HOP_FLAG_FEN | hp.HOP_FLAG_HADME
        far = (0, 0) if i % 4 == 3 else (4 * (px + 40 + 16 * (i % 3)) + 1, 4 * (py + 6) + 2)
        j["n_amvp"] = 2; j["amvp"] = [4 * px, 4 * py, far[0], far[1]]
    return jobs


def reach_above(L, pic_w, job, row_top):
    L.hop_me_reach_above.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.hop_me_reach_above.restype = ctypes.c_int
    j = np.ascontiguousarray(np.array([job], hp.PU_JOB_DTYPE))
    return int(L.hop_me_reach_above(pic_w, j.ctypes.data, row_top))


def formula(pic_w, j, row_top):
    """what hop_me_search reads above row_top, restated: the window with the block, the probes and the taps (half the larger block side + 8 around the block at every
    displacement), and the GT patch (half a block around the displaced block) at every AMVP start vector"""
    w, h = int(j["w"]), int(j["h"])
    m = max(w, h) // 2 + 8
    xs = []
    if int(j["pu_y"]) + int(j["rng_top"]) - m < row_top:
        xs.append(int(j["pu_x"]) + int(j["rng_right"]) + w + m)
    for k in range(int(j["n_amvp"])):
        ax, ay = int(np.int16(j["amvp"][2 * k])), int(np.int16(j["amvp"][2 * k + 1]))
        if (ax, ay) == (0, 0): continue
        if int(j["pu_y"]) + (ay >> 2) - h // 2 < row_top:
            xs.append(int(j["pu_x"]) + (ax >> 2) + w + w // 2)
    return min(max(xs), pic_w - 1) >> 6 if xs else -1


def test_the_wait_column_is_the_formulas():
    L = hp.load()
    jobs = bound_jobs()
    cols = [reach_above(L, BOUND_W, j, 64) for j in jobs]
    assert cols == [formula(BOUND_W, j, 64) for j in jobs]
    assert len(set(cols)) >= 4 and min(cols) >= 0 and max(cols) <= 6     # several different columns, none of them beyond the picture
    # the far AMVP vector moves the column where it points beyond the window, and only there
    moved = 0
    for j in jobs:
        k = j.copy(); k["n_amvp"] = 1
        a, b = reach_above(L, BOUND_W, j, 64), reach_above(L, BOUND_W, k, 64)
        assert a >= b
        moved += a > b
    assert moved >= 3
    # random jobs, windows above and below the row's top, clipped at the picture's right edge
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(400):
        j = np.zeros(1, hp.PU_JOB_DTYPE)[0]
        w, h = [int(v) for v in rng.choice([4, 8, 16, 32, 64], 2)]
        j["w"], j["h"], j["pu_x"], j["pu_y"] = w, h, 4 * int(rng.integers(0, (BOUND_W - w) // 4 + 1)), 64 + 4 * int(rng.integers(0, (64 - h) // 4 + 1))
        l, t = int(rng.integers(-128, 100)), int(rng.integers(-120, 20))
        j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"] = l, l + int(rng.integers(0, 60)), t, t + int(rng.integers(0, 60))
        j["n_amvp"] = int(rng.integers(0, 3))
        j["amvp"] = [int(v) for v in rng.integers(-600, 600, 4)]
        got = reach_above(L, BOUND_W, j, 64)
        assert got == formula(BOUND_W, j, 64), j
        seen.add(got)
    assert {-1, 0, 6} <= seen
