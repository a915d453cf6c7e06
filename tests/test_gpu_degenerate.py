"""GPU: ties and saturation.  Every search kernel promises the reference's first-best choice (strict `<` in the reference's visit order); how a kernel keeps that promise
-- packed atomicMin keys, per-lane incumbents, pruning against a running best, candidate order -- is exercised only when two candidates cost exactly the same, and the
clips of the filters only when samples sit at the ends of the range.  The noisy synthetic lenslets of the other modules almost never do either.  Here: the degenerate
pictures of tests/degenerate.py (flat, exactly periodic, two-level, clipped) through every search, against what the REFERENCE's own code did on them
(tests/golden/degenerate.npz, oracle/make_golden25.py) and against the restatement, which tests/test_degenerate_cpu.py pins to the same golden.  That module also
asserts the shares of ties and clips the golden holds.  Bit-exact everywhere."""
import ctypes
import functools
import importlib.util
import os
import tempfile

import numpy as np
import pytest

import degenerate as dg
from goldutil import load
from hoputil import ROOT, SAO_PARAM_DTYPE, Planes, lambda_for_qp, oracle, oracle_deblock, p16
from test_degenerate_cpu import INTRA_KEYS, intra_case, me_scenarios, pred_case, spine_view
from test_spine_cpu import check_against_golden, cpu_last_levels, cpu_last_rd_fraction, levels_match_cbf, run_cpu, run_cpu_wpp, spine_cpu

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p
LEAF_SWITCHES = ("HOP_FUSED_LEAF", "HOP_WALK")


def _hophip():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module", params=["leaf-fused", "leaf-staged"])
def hp(request):
    """the transform, intra and quadtree parts twice, as tests/test_gpu_tq_intra.py runs them: the transform-unit leaf step as one kernel per batch and the candidate chains
    as one walk kernel per candidate (the defaults), and both as staged batch steps (HOP_FUSED_LEAF=0 HOP_WALK=0, read when a context is created)"""
    m = _hophip()
    old = [os.environ.get(k) for k in LEAF_SWITCHES]
    for k in LEAF_SWITCHES:
        if request.param == "leaf-staged":
            os.environ[k] = "0"
        else:
            os.environ.pop(k, None)
    yield m
    for k, v in zip(LEAF_SWITCHES, old):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture
def hp0(monkeypatch):
    """the library with none of the leaf switches set, whatever the `hp` fixture of this module left in the environment"""
    for k in LEAF_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return _hophip()


@pytest.fixture(scope="module")
def G():
    return load("degenerate.npz")


def _jobs_from_golden(hp, jobs, lc):
    a = np.zeros(len(jobs), hp.PU_JOB_DTYPE)
    for i, job in enumerate(jobs):
        (_, puX, puY, w, h, cuX, cuY, cuS, offx, offy, fr, fc, px, py, l, r, t, b, ox, oy, nA) = [int(v) for v in job[:21]]
        a[i]["pu_x"], a[i]["pu_y"], a[i]["w"], a[i]["h"] = puX, puY, w, h
        a[i]["rng_left"], a[i]["rng_right"], a[i]["rng_top"], a[i]["rng_bottom"] = l, r, t, b
        a[i]["off_x"], a[i]["off_y"], a[i]["pred_x"], a[i]["pred_y"] = ox, oy, px, py
        a[i]["lambda_cost"], a[i]["n_amvp"] = lc, nA
        a[i]["amvp"] = [int(v) for v in job[21:25]]
        a[i]["flags"] = hp.HOP_FLAG_FEN | hp.HOP_FLAG_HADME
    return a


def _res_row(r):
    """hop_pu_result -> the 27-entry layout of oracle/ref_harness.cpp:ref_me_pu"""
    return ([int(r["mv_int"][0]), int(r["mv_int"][1]), int(r["sad"]), int(r["not_valid"])] + [int(v) for v in r["half"]] +
            [int(v) for v in r["qter"]] + [int(r["frac_cost"]), int(r["gt_flag"])] + [int(v) for v in r["gt"]] +
            [int(r["cost"])] + [int(v) for v in r["mv_final"]] + [int(v) for v in r["half_final"]] + [int(v) for v in r["qter_final"]] +
            [int(r["mv_int"][0]), int(r["mv_int"][1])])


# ---- a. the ME chain against the golden ----
@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("name", dg.ME_PICTURES)
def test_me_chain_on_degenerate_pictures(hp0, G, name, stage):
    """SS search / + fractional / + GT against the reference on 32 PUs per picture (24 shapes incl. AMP, first-row and first-column CUs, partly coded CTUs)"""
    ctx, n = None, 0
    for pl, Y, Cb, Cr, jobs, outs, _, lc in me_scenarios(G, name):
        if ctx is None:
            ctx = hp0.Context(pl.W, pl.H)
            ctx.upload_orig(Y, Cb, Cr)
        for c, b in enumerate((pl.bufY, pl.bufCb, pl.bufCr)):
            ctx.ssref_upload(c, b)
        res = ctx.me_search(_jobs_from_golden(hp0, jobs, lc), stage)
        for job, r, want in zip(jobs, res, outs):
            got, want = _res_row(r), [int(v) for v in want]
            n += 1
            if want[3]:                      # not valid: only the integer stage is defined
                assert got[2:4] == want[2:4], (name, job, got, want)
                continue
            assert got[0:4] == want[0:4], (name, job, got, want)
            if stage >= 2:
                assert got[4:9] == want[4:9], (name, job, got, want)
            if stage >= 3:
                assert got[9:25] == want[9:25], (name, job, got, want)
    ctx.close()
    assert n == 32                           # no PU is left out


@pytest.mark.parametrize("name", dg.ME_PICTURES)
def test_me_chain_developer_switches_do_not_change_a_byte(hp0, G, name, monkeypatch):
    """stage 3: shared family passes on / off, one and three stream lanes"""
    scen = list(me_scenarios(G, name))
    outs = []
    for env in ({}, {"HOP_SS_FAMILIES": "0"}, {"HOP_SS_FAMILIES": "1"}, {"HOP_LANES": "1"}, {"HOP_LANES": "3"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            ctx = hp0.Context(dg.ME_W, dg.ME_H)
        ctx.upload_orig(*scen[0][1:4])
        got = b""
        for pl, _, _, _, jobs, _, _, lc in scen:
            for c, b in enumerate((pl.bufY, pl.bufCb, pl.bufCr)):
                ctx.ssref_upload(c, b)
            got += ctx.me_search(_jobs_from_golden(hp0, jobs, lc), 3).tobytes()
        ctx.close()
        outs.append(got)
    assert all(o == outs[0] for o in outs[1:])


# ---- b. families and cells on tied content, against the restatement ----
FAMILY_CUS = [(128, 128, 64), (64, 128, 64), (128, 128, 32), (160, 160, 32), (128, 128, 16), (176, 144, 16), (240, 176, 16), (128, 128, 8), (200, 136, 8), (0, 128, 8), (248, 184, 8),
              (128, 0, 16)]


@pytest.mark.parametrize("flags", ["fen_hadme", "fen", "none"])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", ["flat_mid", "tile15"])
def test_ss_families_and_cells_on_tied_content(hp0, name, bd, flags, monkeypatch):
    """the five-member families of test_ss_families_vs_oracle and one whole-CTU enumeration (425 PUs, hop_enumerate_ctu_jobs) at stage 1 on a flat and on an exactly
    15-periodic picture: a sentinel hole inside the coded area, the uncoded area next to it, common and per-member predictors -- among them multiples of 4, around which
    +dx and -dx carry the same number of bits.  Every PU against the restatement; HOP_SS_FAMILIES=0 must give the same bytes."""
    O = oracle()
    flags = {"fen_hadme": hp0.HOP_FLAG_FEN | hp0.HOP_FLAG_HADME, "fen": hp0.HOP_FLAG_FEN, "none": 0}[flags]
    W, H = 256, 192
    Y, Cb, Cr = dg.picture(name, W, H, bd)
    rng = np.random.default_rng(700 + bd + flags)
    pl = Planes(W, H)
    pl.y00()[:128, :W] = Y[:128]
    pl.y00()[128:192, :128] = Y[128:192, :128]
    pl.y00()[70:84, 100:140] = -1                    # a hole of sentinels inside the coded area
    # border extension, as goldutil.coded_planes does it (re-commit the 8x8 block at (0,0) with the values it holds): while the first sample of the padded plane is still
    # the sentinel every PU is not valid (TEncSearch.cpp:4603-4606) and only its cost would be compared, not the vector that a tie decides
    O.hop_o_ssref_commit_cu(pl.ptr00(0), pl.ptr00(1), pl.ptr00(2), W, H, 0, 0, 8, p16(np.ascontiguousarray(pl.y00()[0:8, 0:8])),
                            p16(np.ascontiguousarray(pl.bufCb[40:44, 40:44])), p16(np.ascontiguousarray(pl.bufCr[40:44, 40:44])))
    lam, lc = lambda_for_qp(int(rng.integers(22, 38)))
    fam =np.zeros(5 * len(FAMILY_CUS), hp0.PU_JOB_DTYPE)
    for c, (cuX, cuY, S) in enumerate(FAMILY_CUS):
        h = S // 2
        common = (4 * int(rng.integers(-12, 12)), 4 * int(rng.integers(-50, -8))) if c % 4 == 0 else (int(rng.integers(-50, 50)), int(rng.integers(-200, -30)))
        for m, (ox, oy, w, hh) in enumerate(((0, 0, S, S), (0, 0, h, S), (h, 0, h, S), (0, 0, S, h), (0, h, S, h))):
            pred = common if c % 2 == 0 else (int(rng.integers(-60, 60)), int(rng.integers(-220, -20)))
            if c % 2 and m == 2:
                pred = (pred[0] & ~3, pred[1] & ~3)
            o6 = (ctypes.c_int * 6)()
            O.hop_o_set_search_range(W, H, cuX, cuY, S, (cuY // 64) * 4 + cuX // 64, 4, pred[0], pred[1], 128, ox, oy, int(cuY == 0), int(cuX == 0), o6)
            j = fam[5 * c + m]
            j["pu_x"], j["pu_y"], j["w"], j["h"] = cuX + ox, cuY + oy, w, hh
            j["rng_left"], j["rng_right"], j["rng_top"], j["rng_bottom"], j["off_x"], j["off_y"] = list(o6)
            j["pred_x"], j["pred_y"], j["lambda_cost"], j["n_amvp"] = pred[0], pred[1], lc, 0
            j["flags"] = flags
    cell = np.zeros(425, hp0.PU_JOB_DTYPE)
    L = hp0.load()
    assert L.hop_enumerate_ctu_jobs(W, H, 2 * 4 + 2, 128, (ctypes.c_int * 2)(4, -72), 0, None, lc, flags, 0, cell.ctypes.data, None, 425) == 425
    jobs = np.concatenate([fam, cell])
    outs = []
    for switch in ("1", "0"):
        with monkeypatch.context() as m:
            m.setenv("HOP_SS_FAMILIES", switch)
            ctx = hp0.Context(W, H, bit_depth=bd)
        ctx.upload_orig(Y, Cb, Cr)
        ctx.ssref_upload(0, pl.bufY)
        outs.append(ctx.me_search(jobs, 1).copy())
        ctx.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    valid = 0
    for j, r in zip(jobs, outs[0]):
        out = (ctypes.c_int64 * 32)()
        org = np.ascontiguousarray(Y[j["pu_y"]:j["pu_y"] + j["h"], j["pu_x"]:j["pu_x"] + j["w"]])
        O.hop_o_me_pu(p16(org), int(j["w"]), pl.ptr00(0), pl.sy, int(j["pu_x"]), int(j["pu_y"]), int(j["w"]), int(j["h"]),
                      int(j["rng_left"]), int(j["rng_right"]), int(j["rng_top"]), int(j["rng_bottom"]), int(j["off_x"]), int(j["off_y"]),
                      int(j["pred_x"]), int(j["pred_y"]), 0, (ctypes.c_int * 4)(0, 0, 0, 0), lc,
                      1 if flags & hp0.HOP_FLAG_FEN else 0, 1 if flags & hp0.HOP_FLAG_HADME else 0, bd, 1, out)
        want, got = list(out)[:27], _res_row(r)
        where = (name, bd, flags, [int(j[k]) for k in ("pu_x", "pu_y", "w", "h", "pred_x", "pred_y")], got[:4], want[:4])
        if want[3]:
            assert got[2:4] == want[2:4], where
        else:
            assert got[:4] == want[:4], where
            valid += 1
    assert valid * 2 > len(jobs)


# ---- c. hop_pred_inter against the golden ----
@pytest.mark.parametrize("name", dg.PRED_PICTURES)
def test_pred_inter_on_degenerate_pictures(hp0, G, name):
    """48 jobs per picture (GT and plain, integer and fractional vectors), one call per job; then at least 16 jobs that do not overlap in one call"""
    pl, (Y, Cb, Cr), jobs, wants = pred_case(G, name)
    ctx = hp0.Context(dg.ME_W, dg.ME_H)
    ctx.upload_orig(Y, Cb, Cr)
    for c, b in enumerate((pl.bufY, pl.bufCb, pl.bufCr)):
        ctx.ssref_upload(c, b)
    pjs = []
    for job in jobs:
        j = hp0.PredJob(*[int(v) for v in job[:7]])
        for k in range(8):
            j.gt[k] = int(job[7 + k])
        pjs.append(j)
    for pj, job, want in zip(pjs, jobs, wants):
        assert np.array_equal(np.concatenate(ctx.pred_inter([pj])), want), (name, [int(v) for v in job])
    sel = []
    for i, job in enumerate(jobs):
        x, y, w, h = [int(v) for v in job[:4]]
        if all(x + w <= int(jobs[k][0]) or int(jobs[k][0]) + int(jobs[k][2]) <= x or y + h <= int(jobs[k][1]) or int(jobs[k][1]) + int(jobs[k][3]) <= y for k in sel):
            sel.append(i)
    assert len(sel) >= 16
    oy, ocb, ocr = ctx.pred_inter([pjs[i] for i in sel])
    a = b = 0
    for i in sel:
        n = int(jobs[i][2]) * int(jobs[i][3])
        got = np.concatenate([oy[a:a + n], ocb[b:b + n // 4], ocr[b:b + n // 4]])
        assert np.array_equal(got, wants[i]), (name, "batched", [int(v) for v in jobs[i]])
        a += n; b += n // 4
    ctx.close()


# ---- d. hop_distortion at the extremes ----
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("case", ["0_vs_top", "top_vs_0", "checker1_vs_inverse"])
def test_distortion_at_the_extremes(hp0, case, bd):
    """the largest values the 32-bit accumulators hold: every sample differs by the whole range; every PU shape of test_distortion_vs_oracle, three components"""
    O = oracle()
    W, H = 128, 128
    org = {"0_vs_top": dg.flat(W, H, 0, bd), "top_vs_0": dg.flat(W, H, "top", bd), "checker1_vs_inverse": dg.checker(W, H, 1, bd)}[case]
    org = [org[0]] + ([np.full((H // 2, W // 2), org[0][0, 0], np.int16)] * 2 if case != "checker1_vs_inverse" else [dg.checker(W // 2, H // 2, 1, bd)[0]] * 2)
    prd = [(dg.top_of(bd) - a).astype(np.int16) for a in org]
    ctx = hp0.Context(W, H, bit_depth=bd)
    ctx.upload_orig(*org)
    for c in range(3):
        ctx.plane_upload("pred", c, prd[c])
    dj, want = [], []
    for (x, y, w, h) in ((0, 0, 64, 64), (64, 32, 32, 16), (8, 8, 8, 8), (16, 4, 16, 4), (32, 64, 12, 16), (4, 4, 8, 4), (0, 64, 64, 48)):
        for comp in range(3):
            ww, hh, xx, yy = (w, h, x, y) if comp == 0 else (w // 2, h // 2, x // 2, y // 2)
            if ww % 4 or hh % 4:
                continue
            a = np.ascontiguousarray(org[comp][yy:yy + hh, xx:xx + ww]); b = np.ascontiguousarray(prd[comp][yy:yy + hh, xx:xx + ww])
            for kind, v in ((hp0.HOP_DIST_SAD, O.hop_o_sad(p16(a), ww, p16(b), ww, ww, hh, bd, 0)), (hp0.HOP_DIST_SSE, O.hop_o_sse(p16(a), ww, p16(b), ww, ww, hh, bd)),
                            (hp0.HOP_DIST_HADS, O.hop_o_hads(p16(a), ww, p16(b), ww, ww, hh, bd))):
                dj.append(hp0.DistJob(x, y, w, h, comp, kind)); want.append(v)
    got = ctx.distortion(dj)
    assert [int(v) for v in got] == [int(v) for v in want]
    assert max(want) >= 64 * 64 * 255 * 255
    ctx.close()


# ---- e. intra rough search and prediction ----
def _intra_jobs(hp, jobs, flags):
    out = []
    for (x, y, N, strong), fl in zip(jobs, flags):
        j = hp.IntraJob(int(x), int(y), int(N), int(strong))
        for k in range(68):
            j.flags[k] = int(fl[k])
        out.append(j)
    return out


@pytest.mark.parametrize("key", INTRA_KEYS)
def test_intra_rough_on_degenerate_pictures(hp, G, key):
    rec, org, jobs, flags, satd = intra_case(G, key)
    ctx = hp.Context(dg.INTRA_W, dg.INTRA_H)
    z = np.zeros((dg.INTRA_H // 2, dg.INTRA_W // 2), np.int16)
    ctx.upload_orig(org, z, z)
    ctx.plane_upload("recon", 0, rec)
    got = ctx.intra_rough(_intra_jobs(hp, jobs, flags))
    assert np.array_equal(got, satd), np.argwhere(got != satd)[:5]
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", ["binary", "flat_top"])
def test_intra_pred_on_saturated_reconstructions(hp, G, name, bd):
    """hop_intra_pred: all 35 modes x all five sizes on reconstructions whose samples are 0 or top (the clips of the DC, horizontal and vertical edge filters are reached),
    the blocks, availability kinds and smoothing switches of the golden set, against the restatement's predictor"""
    O = oracle()
    W, H = dg.INTRA_W, dg.INTRA_H
    rec = np.ascontiguousarray(dg.picture(name, W, H, bd)[0])
    _, _, jobs, flags, _ = intra_case(G, "binary_same")
    ctx = hp.Context(W, H, bit_depth=bd)
    z = np.zeros((H // 2, W // 2), np.int16)
    ctx.upload_orig(rec, z, z)
    ctx.plane_upload("recon", 0, rec)
    top = dg.top_of(bd)
    for N in (4, 8, 16, 32, 64):
        mine = [i for i in range(len(jobs)) if int(jobs[i][2]) == N]
        assert len(mine) == 6                                             # the six availability kinds
        lo = hi = 0
        for mode in range(35):
            i = mine[mode % 6]
            x, y, _, strong = [int(v) for v in jobs[i]]
            ctx.intra_pred(_intra_jobs(hp, jobs[i:i + 1], flags[i:i + 1]), [mode])           # (blocks of one call must not overlap in the prediction picture)
            got = ctx.pred_download(0)[y:y + N, x:x + N]
            L = (ctypes.c_int * (4 * 64 + 8))(); F = (ctypes.c_int * (4 * 64 + 8))()
            fla = np.ascontiguousarray(flags[i], np.uint8)
            O.hop_o_intra_fill_refs(p16(rec), W, x, y, N, fla.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), bd, L)
            O.hop_o_intra_smooth(L, N, bd, strong, F)
            want = np.zeros((N, N), np.int16)
            O.hop_o_intra_pred(L, F, N, mode, bd, p16(want))
            assert np.array_equal(got, want), (name, bd, x, y, N, mode)
            lo += int((want == 0).any()); hi += int((want == top).any())
        assert hi >= 1 and (lo >= 1 or name == "flat_top"), (name, bd, N, lo, hi)
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", ["binary", "flat_top"])
def test_intra_pred_chroma_on_saturated_reconstructions(hp, name, bd):
    """hop_intra_pred_chroma: the five chroma candidates (planar, vertical, horizontal, DC and 34, which stands in for a derived mode) x every chroma block size, random
    availability per 2-sample unit, with test_intra_pred_chroma_vs_oracle's harness"""
    O = oracle()
    rng = np.random.default_rng(33 + bd)
    W, H = dg.INTRA_W, dg.INTRA_H
    rec = dg.picture(name, W, H, bd)
    if name == "flat_top":
        rec = (rec[0], np.full_like(rec[1], dg.top_of(bd)), np.full_like(rec[2], dg.top_of(bd)))
    ctx = hp.Context(W, H, bit_depth=bd)
    ctx.upload_orig(*rec)
    for k in range(3):
        ctx.plane_upload("recon", k, rec[k])
    top = dg.top_of(bd)
    for N in (4, 8, 16, 32):
        lo = hi = 0
        for mode in (0, 26, 10, 1, 34):
            for trial in range(3):
                cx, cy = int(rng.integers(0, (W // 2 - N) // 4 + 1)) * 4, int(rng.integers(0, (H // 2 - N) // 4 + 1)) * 4
                U = N // 2
                fl = np.zeros(68, np.uint8)
                for u in range(4 * U + 1):
                    if u < 2 * U: ok = cx > 0 and cy + 2 * (2 * U - 1 - u) + 2 <= H // 2
                    elif u == 2 * U: ok = cx > 0 and cy > 0
                    else: ok = cy > 0 and cx + 2 * (u - 2 * U - 1) + 2 <= W // 2
                    fl[u] = int(ok and rng.random() < 0.8)
                j = hp.IntraJob(2 * cx, 2 * cy, N, 0)
                for k in range(68): j.flags[k] = int(fl[k])
                ctx.intra_pred_chroma([j], [mode])
                for comp in (1, 2):
                    got = ctx.pred_download(comp)[cy:cy + N, cx:cx + N]
                    L = (ctypes.c_int * (4 * 64 + 8))()
                    O.hop_o_intra_fill_refs_u(p16(np.ascontiguousarray(rec[comp])), W // 2, cx, cy, N, 2, fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), bd, L)
                    want = np.zeros((N, N), np.int16)
                    O.hop_o_intra_pred_chroma(L, N, mode, bd, p16(want))
                    assert np.array_equal(got, want), (name, bd, N, cx, cy, mode, comp)
                    lo += int((want == 0).any()); hi += int((want == top).any())
        assert hi >= 1 and (lo >= 1 or name == "flat_top"), (name, bd, N, lo, hi)
    ctx.close()


# ---- g. whole pictures ----
@functools.lru_cache(maxsize=None)
def _cpu_spine(key):
    """the CPU spine's reconstruction, levels and rd fractions for a spine picture: computed once, shared by the cases of the picture"""
    _, name, W, H, wpp = [f for f in dg.SPINE_FRAMES if f[0] == key][0]
    L = spine_cpu()
    pic = dg.picture(name, W, H)
    rec = run_cpu_wpp(L, W, H, *pic, 0)[4] if wpp else run_cpu(L, W, H, *pic)[4]
    n = ((W + 63) // 64) * ((H + 63) // 64)
    return rec, cpu_last_levels(L, n), cpu_last_rd_fraction(L, n)


SPINE_CASES = [(key, slots, lag) for key, _, _, _, wpp in dg.SPINE_FRAMES for slots in (0, 48) for lag in ((0, 5) if wpp else (None,))]


@pytest.mark.parametrize("key,slots,lag", SPINE_CASES)
def test_encode_decode_and_loop_filters_on_degenerate_pictures(hp0, G, key, slots, lag):
    """hop_encode_frame against the reference encoder's candidate trace, per-CTU costs and partition data; reconstruction, levels, rd fraction and SS reference against the
    CPU spine; hop_decode_frame (both schedules) from the returned parts and levels; then deblocking and SAO against the restatement.  On a flat picture every SAO
    statistic is zero: the parameter decision itself is a tie."""
    hp = hp0
    O = oracle()
    _, name, W, H, wpp = [f for f in dg.SPINE_FRAMES if f[0] == key][0]
    Y, Cb, Cr = dg.picture(name, W, H)
    assert dg.pic_crc((Y, Cb, Cr)) == int(G["spine/%s/pic_crc" % key])
    ctx = hp.Context(W, H, slots=slots)
    ctx.upload_orig(Y, Cb, Cr)
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        cost, bits, dist, parts, nc = ctx.encode_frame(32, 16, 0, tp, wpp=1, wavefront_lag=lag) if wpp else ctx.encode_frame(32, 16, 0, tp)
        text = open(tp, "rb").read()
    pv = parts.view(np.dtype(parts.dtype.descr))
    check_against_golden(spine_view(G), key, cost, bits, dist, pv, text)
    rec, levels, fraction = _cpu_spine(key)
    got = [ctx.recon_download(c) for c in range(3)]
    for c in range(3):
        assert np.array_equal(got[c], rec[c]), (key, c)
    lv = ctx.levels_download()
    assert np.array_equal(lv, levels) and levels_match_cbf(lv, pv) > 0
    assert np.array_equal(ctx.rd_fraction_download(), fraction)
    ss = [ctx.ssref_download(c) for c in range(3)]
    assert np.array_equal(ss[0][80:80 + H, 80:80 + W], rec[0])
    # the decoder, from the syntax alone
    d = hp.Context(W, H)
    for schedule in (0, 1):
        d.decode_frame(parts, lv, qp=32, schedule=schedule)
        for c in range(3):
            assert np.array_equal(d.recon_download(c), rec[c]), (key, "decode", schedule, c)
            assert np.array_equal(d.ssref_download(c), ss[c]), (key, "decode ssref", schedule, c)
    d.close()
    # deblocking
    want = oracle_deblock(W, H, (32, 0, 0, 0, 0), parts, rec)
    ctx.deblock_frame(parts, 32)
    dbk = [ctx.recon_download(c) for c in range(3)]
    for c in range(3):
        assert np.array_equal(dbk[c], want[c]), (key, "deblock", c)
    # SAO: statistics, decision, offsetting
    n, wc = len(cost), (W + 63) // 64
    src = [np.ascontiguousarray(a, np.int16) for a in dbk]; org = [np.ascontiguousarray(a, np.int16) for a in (Y, Cb, Cr)]
    psrc = (VP * 3)(*[a.ctypes.data for a in src]); porg = (VP * 3)(*[a.ctypes.data for a in org])
    stats = np.zeros((n, 3, 5, 32, 2), np.int32)
    assert O.hop_o_sao_stats(W, H, 8, psrc, porg, stats.ctypes.data_as(VP)) == 0
    assert np.array_equal(ctx.sao_stats(), stats)
    lam = lambda_for_qp(32)[0]
    frac = int(fraction[-1])
    coded = ctx.sao_frame([lam, lam, lam], 3, 32, frac)
    p = hp.SaoParams((ctypes.c_double * 3)(lam, lam, lam), (ctypes.c_int32 * 3)(1, 1, 1), 3, 32, frac)
    c2 = np.zeros((n, 3), SAO_PARAM_DTYPE); recon = np.zeros((n, 3), SAO_PARAM_DTYPE)
    ctx.L.hop_sao_decide.argtypes = [ctypes.c_int] * 3 + [VP] * 4
    assert ctx.L.hop_sao_decide(n, wc, 8, stats.ctypes.data, ctypes.addressof(p), c2.ctypes.data, recon.ctypes.data) == 0
    assert coded.tobytes() == c2.tobytes()
    out = [np.zeros_like(a) for a in src]; pout = (VP * 3)(*[a.ctypes.data for a in out])
    assert O.hop_o_sao_apply(W, H, 8, psrc, recon.ctypes.data_as(VP), pout) == 0
    for c in range(3):
        assert np.array_equal(ctx.recon_download(c), out[c]), (key, "sao", c)
    print(key, "slots", slots, "lag", lag, nc, "candidates")
    ctx.close()


# ---- f. transform leaf and quadtree searches on zero, maximal and single-spike residuals, against the restatement ----
QPS = (20, 32, 42)                                         # (+ 6 (bd - 8)), dealt to the CUs of a call in turn
CONTENTS = ["zero", "max", "spike"]


def _block(kind, rng, n, bd, inner=None, one_level=False):
    """original and what it is predicted from, n x n: zero -- both the same flat value (every candidate has distortion 0: bits and order decide); max -- a two-level
    0 / top pattern against its inverse (residuals of +-top at every transform size); spike -- flat, with a single sample at the other end of the range"""
    top, mid = dg.top_of(bd), dg.mid_of(bd)
    v = int(rng.choice([0, mid, top]))
    if kind == "zero":
        a = np.full((n, n), v, np.int16)
        return a, a.copy()
    if kind == "max":
        k = int(rng.choice([1, 2, 4, 8, 64]))           # squares of k samples; 64 (or one_level): one level over the whole block, the largest DC coefficient there is:
        if one_level: k = 64                            # about top * n / Qstep = 1285 at n = 32, QP 20 (+ 6 per extra bit), so a level >= 1024 is certain to be offered
        yy, xx = np.mgrid[0:n, 0:n]
        a = ((((yy // k) + (xx // k) + int(rng.integers(0, 2))) & 1) * top).astype(np.int16)
        return a, (top - a).astype(np.int16)
    b = np.full((n, n), v, np.int16)
    a = b.copy()
    lo, hi = (0, n) if inner is None else (1, 1 + inner)             # (inner: the spike inside the CU, which lies at (1, 1) of the block)
    a[int(rng.integers(lo, hi)), int(rng.integers(lo, hi))] = 0 if v == top else top if v == 0 else int(rng.choice([0, top]))
    return a, b


def _inter_content(kind):
    calls = [0]

    def content(rng, cu, bd):
        one = calls[0] % 3 == 0; calls[0] += 1         # the builders call once per CU and deal QPS in turn: every CU at QP 20 is one level against its inverse
        pairs = [_block(kind, rng, cu, bd, one_level=one), _block(kind, rng, cu // 2, bd, one_level=one), _block(kind, rng, cu // 2, bd, one_level=one)]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    return content


def _intra_content(kind, chroma=False):
    calls = [0]

    def content(rng, cu, bd):
        one = (calls[0] // (2 if chroma else 1)) % 3 == 0; calls[0] += 1       # (the chroma builder calls twice per CU)
        n = (cu + 1) if chroma else (2 * cu + 1)       # from (-1, -1) of the CU: the original inside it, what it is predicted from around it
        return _block(kind, rng, n, bd, inner=(cu // 2) if chroma else cu, one_level=one)
    return content


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", CONTENTS)
def test_rqt_on_degenerate_residuals(hp, kind, bd):
    """hop_rqt + hop_rqt_finish, 32 CUs per call (every CU size, sign hiding and transform skip on and off, the inter_split_flag tree), with test_rqt_random_vs_oracle's
    harness"""
    from test_gpu_tq_intra import rqt_random_check
    st = rqt_random_check(hp, bd, content=_inter_content(kind), qps=QPS)
    print("hop_rqt", kind, bd, st)
    if kind == "zero":
        assert st["zeros"] >= 1                                          # the root-cbf-zero test wins
    if kind == "max":
        assert st["big"] >= 1                                            # a level of magnitude >= 1024 survives


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", CONTENTS)
def test_intra_rqt_on_degenerate_residuals(hp, kind, bd):
    """hop_intra_rqt, 72 PUs per call (every CU size, NxN, bCheckFirst, deeper trees, random availability), with test_intra_rqt_random_vs_oracle's harness"""
    from test_gpu_tq_intra import intra_rqt_random_check
    st = intra_rqt_random_check(hp, bd, content=_intra_content(kind), qps=QPS)
    print("hop_intra_rqt", kind, bd, st)
    if kind == "max":
        assert st["big"] >= 1


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", CONTENTS)
def test_intra_luma_search_on_degenerate_residuals(hp, kind, bd):
    """hop_intra_luma_search, 72 CUs per call, with test_intra_luma_search_random_vs_oracle's harness.  In the zero class the neighbourhood is flat: every mode predicts the
    same block, so the candidates of a CU differ in their mode bits alone"""
    from goldutil import oracle_intra_rqt
    from test_gpu_tq_intra import intra_luma_search_random_check
    ties = []

    def two_candidates(cfg, syn, ts_fast, strong, sj, avail, org, win, coder, cu_ctx):
        """a 2Nx2N CU's second and third most probable mode -- candidates of every search -- through the restatement's candidate evaluation (bCheckFirst): equal cost?"""
        if kind != "zero" or syn["part_nxn"]:
            return
        left, above = int(sj["left_dir"][0]), int(sj["above_dir"][0])
        if left == above:
            preds = [left, ((left + 29) % 32) + 2, ((left - 1) % 32) + 2] if left > 1 else [0, 1, 26]
        else:
            preds = [left, above, 0 if (left and above) else (26 if left + above < 2 else 1)]
        s2 = syn.copy(); s2["preds"][0] = preds; s2["pred_num"][0] = 3
        costs = []
        for mode in preds[1:]:
            s2["luma_dir"][0] = mode
            costs.append(oracle_intra_rqt(cfg, s2, [0, 0, 1, ts_fast, strong], avail, org, win, np.zeros(1792, np.uint8), coder, cu_ctx)[0])
        ties.append(costs[0] == costs[1])
    st = intra_luma_search_random_check(hp, bd, on_cu=two_candidates, content=_intra_content(kind), qps=QPS)
    print("hop_intra_luma_search", kind, bd, st, "CUs whose second and third most probable mode cost the same:", sum(ties), "of", len(ties))
    assert st["nxn"] >= 4
    if kind == "zero":
        assert sum(ties) >= 1                                            # two candidates of equal cost: the first one tested must have won
    if kind == "max":
        assert st["big"] >= 1


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", CONTENTS)
def test_intra_chroma_search_on_degenerate_residuals(hp, kind, bd):
    """hop_intra_luma_search followed by hop_intra_chroma_search, 72 CUs per call, luma and both chroma planes of the same class, with
    test_intra_chroma_search_random_vs_oracle's harness.  A chroma transform unit is at most 16 x 16 (a 64 CU has four): one level against its inverse gives a DC level
    of about top * 16 / Qstep = 642 at QP 20 (+ 6 per extra bit), more where the plane's QP offset lowers the quantiser; 1024 needs an offset of 5, which the harness
    draws for one plane in six (measured: one CU at 8 bit, none at 10 bit).  So the condition here is a chroma level >= 512, which every one-level CU of 32 or 64 at the
    lowest QP offers; the levels >= 1024 are the luma entries' to reach"""
    from test_gpu_tq_intra import intra_chroma_search_random_check
    st = intra_chroma_search_random_check(hp, bd, chroma_content=_intra_content(kind, True), content=_intra_content(kind), qps=QPS)
    print("hop_intra_chroma_search", kind, bd, st)
    if kind == "max":
        assert st["peak"] >= 512


@pytest.mark.parametrize("sign_hide", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_tu_roundtrip_on_degenerate_residuals(hp, bd, sign_hide):
    """hop_tu_roundtrip without and with sign hiding: every TU size, DCT / DST / transform skip, three components, both rounding offsets, on zero, maximal (two-level
    against its inverse: the 16-bit clips of the inverse path) and single-spike residuals"""
    O = oracle()
    O.hop_o_tu_roundtrip_sbh.restype = ctypes.c_uint32
    W, H = 128, 128
    rng = np.random.default_rng(5 + bd + sign_hide)
    top, mid = dg.top_of(bd), dg.mid_of(bd)
    org = [np.full((H >> (c > 0), W >> (c > 0)), mid, np.int16) for c in range(3)]; prd = [a.copy() for a in org]
    jobs = []
    for kind in CONTENTS:
        for log2 in (2, 3, 4, 5):
            N = 1 << log2
            for comp in (0, 1, 2):
                for k in range(4):
                    qp = QPS[(k + log2) % 3] + 6 * (bd - 8)
                    scan = int(rng.integers(0, 3)) if (sign_hide and log2 <= 3) else 0
                    jobs.append((kind, comp, log2, int(log2 == 2 and comp == 0 and k % 2 == 0), int(log2 == 2 and k == 3), qp, k % 2, scan))
    # each job in a 32 x 32 cell of its own component plane (chroma planes are 64 x 64: four cells; the jobs run one by one, the cells are reused)
    big = 0
    ctx = hp.Context(W, H, bit_depth=bd)
    for kind, comp, log2, dst, ts, qp, isl, scan in jobs:
        N = 1 << log2
        a, b = _block(kind, rng, N, bd, one_level=(qp == QPS[0] + 6 * (bd - 8)))
        org[comp][0:N, 0:N] = a; prd[comp][0:N, 0:N] = b
        ctx.upload_orig(*org)
        ctx.plane_upload("pred", comp, prd[comp])
        j = hp.TuJob(0, 0, comp, log2, dst, ts, qp, isl, sign_hide, scan)
        res, lv = ctx.tu_roundtrip([j])
        lvo = np.zeros(N * N, np.int32); rec = np.zeros((N, N), np.int16); sse = ctypes.c_uint32()
        s = O.hop_o_tu_roundtrip_sbh(bd, qp, isl, dst, ts, N, sign_hide, scan, p16(np.ascontiguousarray(a)), p16(np.ascontiguousarray(b)), lvo.ctypes.data_as(VP), p16(rec), ctypes.byref(sse))
        assert res[0] == (s, sse.value) and np.array_equal(lv, lvo), (kind, comp, N, dst, ts, qp, res, s, sse.value)
        assert np.array_equal(ctx.recon_download(comp)[0:N, 0:N], rec), (kind, comp, N, dst, ts, qp)
        big += int(np.abs(lvo).max() >= 1024)
    assert big >= 1
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_tu_rd_on_degenerate_residuals(hp, bd):
    """hop_tu_rd (forward transform, RDOQ, counted bits, inverse path, cbf-zero decision) against the restatement's leaf step: every TU size and component of
    test_tu_rd_golden's set at transform depths 0..2, sign hiding and transform skip on and off, zero / maximal / single-spike residuals, each TU with a context
    snapshot of its own and a carried fraction"""
    O = oracle()
    O.hop_o_tu_rd.argtypes = [VP] + [ctypes.c_int] * 7 + [ctypes.c_double] * 3 + [VP, ctypes.c_uint32, VP, VP, VP]
    rng = np.random.default_rng(60 + bd)
    W = H = 256
    mid = dg.mid_of(bd)
    org = [np.full((H >> (c > 0), W >> (c > 0)), mid, np.int16) for c in range(3)]; prd = [a.copy() for a in org]
    cases = [(kind, log2, comp, trd) for kind in CONTENTS for (log2, comp) in [(2, 0), (3, 0), (4, 0), (5, 0), (2, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2)] for trd in (0, 1, 2)]
    jobs = np.zeros(len(cases), hp.TU_RD_JOB_DTYPE); snaps = np.zeros((len(cases), hp.CABAC_CTX_BYTES), np.uint8); resis = []
    L = hp.load()
    L.hop_cabac_init.argtypes = [VP, ctypes.c_int, ctypes.c_int]
    slot = [0, 0, 0]
    for i, (kind, log2, comp, trd) in enumerate(cases):
        N = 1 << log2; k = slot[comp]; slot[comp] += 1
        cell = 32 if comp == 0 else 16
        px, py = cell * (k % 8), cell * (k // 8)
        a, b = _block(kind, rng, N, bd, one_level=(i % 3 == 0))
        org[comp][py:py + N, px:px + N] = a; prd[comp][py:py + N, px:px + N] = b
        resis.append(np.ascontiguousarray((a - b).astype(np.int16).ravel()))
        qp = QPS[i % 3] + 6 * (bd - 8); lam = 0.57 * 2.0 ** ((qp - 6 * (bd - 8) - 12) / 3.0); w = float(rng.choice([1.0, 1.26])) if comp else 1.0
        j = jobs[i]
        j["x"], j["y"] = (px, py) if comp == 0 else (2 * px, 2 * py)
        j["comp"], j["log2_size"], j["qp_scaled"], j["tr_depth"], j["ctx_index"], j["bit_depth"] = comp, log2, qp, trd, i, bd
        j["sign_hide"], j["use_ts"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        j["lambda_rdoq"], j["lambda_rd"], j["dist_weight"] = lam / w, lam, w
        assert L.hop_cabac_init(snaps[i].ctypes.data, int(rng.integers(0, 5)), int(rng.integers(20, 45))) == 0
        left = int(rng.integers(0, 32768)); snaps[i, 150], snaps[i, 151] = left & 255, left >> 8
    assert max(slot) <= 64
    ctx = hp.Context(W, H, bit_depth=bd)
    ctx.upload_orig(*org)
    for comp in range(3):
        ctx.plane_upload("pred", comp, prd[comp])
    res, lv = ctx.tu_rd(jobs, snaps)
    off = big = zero = 0
    for i, (kind, log2, comp, trd) in enumerate(cases):
        j = jobs[i]; n = 1 << (2 * log2)
        lvo = np.zeros(n, np.int32); o = np.zeros(8, np.uint32); cost = ctypes.c_double()
        st = np.ascontiguousarray(snaps[i])
        assert O.hop_o_tu_rd(resis[i].ctypes.data, log2, comp, int(j["qp_scaled"]), bd, trd, int(j["sign_hide"]), int(j["use_ts"]), float(j["lambda_rdoq"]), float(j["lambda_rd"]),
                             float(j["dist_weight"]), st.ctypes.data, int(st[150]) | (int(st[151]) << 8), lvo.ctypes.data, o.ctypes.data, ctypes.byref(cost)) == 0
        got = [int(res[i][k]) for k in ("abs_sum", "cbf", "dist", "zero_dist", "nonzero_dist", "bits", "null_bits")]
        assert got == [int(v) for v in o[:7]], (bd, i, cases[i], got, o)
        assert float(res[i]["cost"]) == cost.value and np.array_equal(lv[off:off + n], lvo), (bd, i, cases[i])
        big += int(np.abs(lvo).max() >= 1024); zero += int(kind == "zero" and o[1] == 0)
        off += n
    assert big >= 1 and zero == 30, (bd, big, zero)
    ctx.close()
