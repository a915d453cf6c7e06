"""CPU: the host half of hop_decode_frame (host/hop_decode.cpp) on the partition data of the CPU spine's golden pictures.

1. the schedule: every CTU's intra neighbours sit in a lower level; for every SS/GT PU every raster-earlier CTU its footprint touches sits in a lower level and every
   raster-later one in a higher level; raster order has one level per CTU, the dependency schedule of the 448x192 picture fewer;
2. the footprint is conservative, by brute force: a CTU whose samples (margins included) change the oracle's prediction of a PU is in the library's footprint;
3. hop_sao_reconstruct_params equals the recon parameters hop_sao_decide returns with the same decision, on every sao_ref.npz case;
4. malformed partition data is refused with HOP_ERR_ARG."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from hoputil import MARGIN_C, MARGIN_Y, ROOT, SAO_PARAM_DTYPE, Planes, lenslet, oracle, sao_cases, sao_params_of
from test_spine_cpu import FRAMES, FRAMES_MI15, FRAMES_WPP, PLAIN, cpu_last_levels, frame, run_cpu, run_cpu_plain, run_cpu_wpp, spine_cpu

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip  # noqa: E402

CASES = ([("frame", W, H, seed, sharp) for W, H, seed, sharp in FRAMES] + [("wpp", W, H, seed, lag) for W, H, seed, lag in FRAMES_WPP if lag]
         + [("mi15", W, H, seed, lag) for W, H, seed, lag in FRAMES_MI15] + [("plain", 136, 72, bd, qp) for bd, qp in PLAIN[:2]])


def case_id(c):
    return "%s_%dx%d_%s_%s" % c


SPINE_REC = {}          # case -> the three planes the CPU spine reconstructed, kept by coded() for tests/test_refdecode_cpu.py


@functools.lru_cache(maxsize=None)
def coded(case):
    """(W, H, parts, levels) of the CPU spine's run on the case's picture"""
    kind, W, H, a, b = case
    L = spine_cpu()
    n = ((W + 63) // 64) * ((H + 63) // 64)
    if kind == "frame":
        Y, Cb, Cr = frame(W, H, a, b)
        out = run_cpu(L, W, H, Y, Cb, Cr)
    elif kind == "wpp":
        Y, Cb, Cr = lenslet(W, H, 16, a)
        out = run_cpu_wpp(L, W, H, Y, Cb, Cr, b)
    elif kind == "mi15":
        Y, Cb, Cr = lenslet(W, H, 15, a)
        out = run_cpu(L, W, H, Y, Cb, Cr, mi=15) if b is None else run_cpu_wpp(L, W, H, Y, Cb, Cr, b, mi=15)
    else:                                                             # the plain intra configurations, at 8 and 10 bit
        rng = np.random.RandomState(9)
        Y, Cb, Cr = lenslet(W, H, 16, 9)
        if a > 8:
            Y, Cb, Cr = (np.clip(p.astype(np.int32) * 4 + rng.randint(0, 4, p.shape), 0, 1023).astype(np.int16) for p in (Y, Cb, Cr))
        out = run_cpu_plain(L, W, H, Y, Cb, Cr, b, a)
    parts, SPINE_REC[case] = out[3], out[4]
    levels = cpu_last_levels(L, n)
    return W, H, np.ascontiguousarray(parts).view(hophip.CU_PART_DTYPE).reshape(n, 256), levels


def zpos(z):
    x = y = 0
    for b in range(4):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def zidx(x4, y4):
    z = 0
    for b in range(4):
        z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1))
    return z


def pu_rect(ps, S, pu):
    ox = oy = 0; w = h = S
    if ps == 1: h = S >> 1; oy = S >> 1 if pu else 0
    elif ps == 2: w = S >> 1; ox = S >> 1 if pu else 0
    elif ps == 3: w = h = S >> 1; ox = S >> 1 if pu & 1 else 0; oy = S >> 1 if pu >> 1 else 0
    elif ps == 4: h = (S >> 2) + (S >> 1) if pu else S >> 2; oy = S >> 2 if pu else 0
    elif ps == 5: h = S >> 2 if pu else (S >> 2) + (S >> 1); oy = (S >> 2) + (S >> 1) if pu else 0
    elif ps == 6: w = (S >> 2) + (S >> 1) if pu else S >> 2; ox = S >> 2 if pu else 0
    elif ps == 7: w = S >> 2 if pu else (S >> 2) + (S >> 1); ox = (S >> 2) + (S >> 1) if pu else 0
    return ox, oy, w, h


def inter_pus(W, H, parts):
    """(CTU, PredJob) of every SS/GT PU, as the decoder predicts it: the vector clipped at the CU (TComDataCU::clipMv), GT for a non-merge PU with its flag"""
    wctu = (W + 63) // 64
    out = []
    for a in range(parts.shape[0]):
        P = parts[a]; cx0, cy0 = (a % wctu) * 64, (a // wctu) * 64
        z = 0
        while z < 256:
            if P["pred_mode"][z] not in (0, 1):
                z += 1; continue
            d = int(P["depth"][z]); S = 64 >> d
            if P["pred_mode"][z] == 0:
                x4, y4 = zpos(z); cx, cy = cx0 + 4 * x4, cy0 + 4 * y4
                ps = int(P["part_size"][z])
                for pu in range({0: 1, 3: 4}.get(ps, 2)):
                    ox, oy, w, h = pu_rect(ps, S, pu)
                    p = P[zidx(((cx & 63) + ox) >> 2, ((cy & 63) + oy) >> 2)]
                    mx = min((W + 8 - cx - 1) * 4, max((-64 - 8 - cx + 1) * 4, int(p["mv"][0])))
                    my = min((H + 8 - cy - 1) * 4, max((-64 - 8 - cy + 1) * 4, int(p["mv"][1])))
                    use = 1 if (not p["merge_flag"] and p["gt_flag"]) else 0
                    j = hophip.PredJob(cx + ox, cy + oy, w, h, mx, my, use, (ctypes.c_int32 * 8)(*[int(v) for v in p["gt"]]), 0)
                    out.append((a, j))
            z += 256 >> (2 * d)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_schedule_keeps_every_dependency(case):
    W, H, parts, _ = coded(case)
    n = parts.shape[0]; wctu = (W + 63) // 64
    lv, nl = hophip.decode_schedule(W, H, parts, 0)
    assert nl == int(lv.max()) + 1 and lv.min() >= 0
    for a in range(n):
        x, y = a % wctu, a // wctu
        for dx, dy in ((-1, 0), (-1, -1), (0, -1), (1, -1)):
            if 0 <= x + dx < wctu and y + dy >= 0:
                assert lv[(y + dy) * wctu + x + dx] < lv[a], (a, dx, dy)
    for a, j in inter_pus(W, H, parts):
        for b in hophip.decode_footprint(W, H, j):
            if b < a: assert lv[b] < lv[a], (a, b)
            if b > a: assert lv[b] > lv[a], (a, b)
    raster, nr = hophip.decode_schedule(W, H, parts, 1)
    assert nr == n and np.array_equal(raster, np.arange(n))
    if (W, H) == (448, 192):
        assert nl < n, (nl, n)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "plain"], ids=case_id)
def test_footprint_is_conservative_by_brute_force(case):
    """every CTU whose samples (its margin replicas included) alter the oracle's prediction of a PU is in the library's footprint (up to 40 PUs per picture, the GT
    ones first)"""
    W, H, parts, _ = coded(case)
    O = oracle()
    wctu = (W + 63) // 64
    pus = inter_pus(W, H, parts)
    pus = sorted(pus, key=lambda t: -t[1].use_gt)[:40]
    if not pus:
        pytest.skip("no SS/GT PU in this picture")
    pl = Planes(W, H)
    rng = np.random.RandomState(W * 7 + H)
    for b in (pl.bufY, pl.bufCb, pl.bufCr):
        b[...] = rng.randint(0, 256, b.shape)
    # the CTU each padded sample belongs to: a margin sample to the CTU of the border sample it replicates
    owners = []
    for b, m, ctu in ((pl.bufY, MARGIN_Y, 64), (pl.bufCb, MARGIN_C, 32), (pl.bufCr, MARGIN_C, 32)):
        ph, pw = b.shape[0] - 2 * m, b.shape[1] - 2 * m
        ry = np.clip(np.arange(b.shape[0]) - m, 0, ph - 1) // ctu
        rx = np.clip(np.arange(b.shape[1]) - m, 0, pw - 1) // ctu
        owners.append(ry[:, None] * wctu + rx[None, :])
    n = parts.shape[0]
    masks = [[np.nonzero(o == k) for o in owners] for k in range(n)]

    def predict(j):
        out = [np.zeros((j.h, j.w), np.int16), np.zeros((j.h // 2, j.w // 2), np.int16), np.zeros((j.h // 2, j.w // 2), np.int16)]
        O.hop_o_pred_inter(pl.ptr00(0), pl.sy, pl.ptr00(1), pl.ptr00(2), pl.sc, j.pu_x, j.pu_y, j.w, j.h, j.mv_x, j.mv_y, j.use_gt, (ctypes.c_int * 8)(*j.gt),
                           8, 8, out[0].ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), out[1].ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                           out[2].ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
        return out

    for a, j in pus:
        fp = set(int(v) for v in hophip.decode_footprint(W, H, j))
        base = predict(j)
        for k in range(n):
            if k in fp:
                continue
            bufs = (pl.bufY, pl.bufCb, pl.bufCr)
            for b, idx in zip(bufs, masks[k]): b[idx] = 255 - b[idx]
            got = predict(j)
            for b, idx in zip(bufs, masks[k]): b[idx] = 255 - b[idx]
            for c in range(3):
                assert np.array_equal(got[c], base[c]), ("PU of CTU %d at (%d, %d) %dx%d gt %d reads CTU %d outside its footprint %s" % (a, j.pu_x, j.pu_y, j.w, j.h, j.use_gt, k, sorted(fp)))


@pytest.mark.parametrize("case", sao_cases(), ids=lambda c: "%s_%dx%d_%dbit" % (c["key"], c["W"], c["H"], c["bd"]))
def test_sao_reconstruct_params_equal_the_decision(case):
    L = hophip.load()
    W, n, bd = case["W"], case["n"], case["bd"]
    coded_ = np.zeros((n, 3), SAO_PARAM_DTYPE); recon = np.zeros((n, 3), SAO_PARAM_DTYPE)
    p = sao_params_of(case)
    L.hop_sao_decide.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    assert L.hop_sao_decide(n, (W + 63) // 64, bd, case["stats"].ctypes.data, ctypes.addressof(p), coded_.ctypes.data, recon.ctypes.data) == 0
    got = hophip.sao_reconstruct_params(coded_.view(hophip.SAO_PARAM_DTYPE), (W + 63) // 64, bd)
    assert got.tobytes() == recon.tobytes()
    bad = coded_.copy().view(hophip.SAO_PARAM_DTYPE); bad[0, 0]["mode"] = 2; bad[0, 0]["type"] = 0     # a merge left in the first CTU has no candidate
    with pytest.raises(hophip.HopError):
        hophip.sao_reconstruct_params(bad, (W + 63) // 64, bd)


def test_malformed_parts_are_refused():
    W, H, parts, _ = coded(("frame", 192, 128, 7, False))
    hophip.decode_schedule(W, H, parts, 0)
    inter = np.argwhere(parts["pred_mode"] == 0)
    intra = np.argwhere(parts["pred_mode"] == 1)
    assert len(inter) and len(intra)

    def refused(mutate):
        p = parts.copy()
        mutate(p)
        with pytest.raises(hophip.HopError):
            hophip.decode_schedule(W, H, p, 0)

    a, u = intra[0]
    refused(lambda p: p[a].__setitem__("luma_dir", np.where(np.arange(256) == u, 35, p[a]["luma_dir"])))
    refused(lambda p: p[a].__setitem__("chroma_dir", np.where(np.arange(256) == u, 40, p[a]["chroma_dir"])))
    deep = np.argwhere((parts["depth"] < 3) & (parts["pred_mode"] != 15) & ((np.arange(256) % 16) == 0)[None, :])
    a2, u2 = deep[0]
    refused(lambda p: p[a2].__setitem__("depth", np.where(np.arange(256) == u2 + 1, p[a2]["depth"][u2] + 1, p[a2]["depth"])))    # depth changes inside a CU
    refused(lambda p: p[a].__setitem__("pred_mode", np.where(np.arange(256) == u, 7, p[a]["pred_mode"])))
    refused(lambda p: p[a].__setitem__("tr_idx", np.where(np.arange(256) == u, 5, p[a]["tr_idx"])))
    b, v = inter[0]
    refused(lambda p: p[b].__setitem__("part_size", np.where(np.arange(256) == v, 9, p[b]["part_size"])))
    refused(lambda p: p[b].__setitem__("part_size", np.where(np.arange(256) == v + 1, (p[b]["part_size"][v] + 1) % 3, p[b]["part_size"])) if v % 4 == 0 else None)
    with pytest.raises(hophip.HopError):
        hophip.decode_schedule(W, H, parts, 2)
