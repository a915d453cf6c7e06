"""CPU: the reference decoder of tests/refdecode.py shown right, and the generated syntax of tests/synthsyntax.py shown to be what it claims.

1. ref_decode of the CPU spine's parts and levels equals the CPU spine's reconstruction on every picture of test_decode_host.CASES (the spine is pinned to the reference
   encoder by encoder_spine.npz), and the interior of its SS reference equals the reconstruction;
2. every item a generated case promises occurs in it (the generator's coverage table), fewer than half of its reference reconstruction is saturated, and
   hop_decode_schedule accepts it."""
import functools
import itertools

import numpy as np
import pytest

import synthsyntax
from hoputil import MARGIN_C, MARGIN_Y
from refdecode import chroma_qp_scaled, ref_decode
from test_decode_host import CASES, SPINE_REC, case_id, coded, hophip


def spine_run(case):
    """the CPU spine's run on the case's picture (test_decode_host.coded, shared with that module's tests) with its reconstruction and the picture's parameters"""
    W, H, parts, levels = coded(case)
    bd, qp, plain = (case[3], case[4], 1) if case[0] == "plain" else (8, 32, 0)
    return W, H, parts, levels, SPINE_REC[case], bd, qp, plain


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_decoder_equals_the_cpu_spine(case):
    W, H, parts, levels, rec, bd, qp, plain = spine_run(case)
    got, ss = ref_decode(W, H, parts, levels, qp, 0, 0, bd, plain)
    for c in range(3):
        assert np.array_equal(got[c], rec[c]), (c, np.argwhere(got[c] != rec[c])[:5])
    if plain:
        assert ss is None
        return
    for c, m in enumerate((MARGIN_Y, MARGIN_C, MARGIN_C)):
        h, w = rec[c].shape
        assert np.array_equal(ss[c][m:m + h, m:m + w], rec[c]), c


# ---- the generated syntax ----
@functools.lru_cache(maxsize=None)
def reference(name):
    """ref_decode of a generated case, once per session (tests/test_gpu_decode_syntax.py shares it); the arrays are not to be written"""
    c = synthsyntax.make_case(name)
    rec, ss = ref_decode(c["W"], c["H"], c["parts"], c["levels"], c["qp"], c["cb_off"], c["cr_off"], c["bd"], c["plain"])
    for a in rec + (ss or []):
        a.setflags(write=False)
    return rec, ss


LEVELS = {("level", s, m) for s in synthsyntax.SHAPES for m in synthsyntax.MAGS}
INTRA_ALL = ({("intra", "luma_dir", N, d) for N in (4, 8, 16, 32) for d in range(35)} | {("intra", "chroma_dir", d) for d in (0, 1, 10, 26, 34, 36, 2, 18, 7, 30)}
             | {("intra", "depth", d) for d in range(4)} | {("intra", "tr_idx", 64, 1), ("intra", "tr_idx", 64, 2), ("intra", "nxn_four_directions"), ("intra", "8x8_2Nx2N_tr1"),
                                                           ("intra", "split_to_4x4", 16), ("intra", "split_to_4x4", 32), ("intra", "tskip", "luma"), ("intra", "tskip", "chroma")}
             | {("intra", "cbf") + t for t in itertools.product((0, 1), repeat=3)} | LEVELS)
INTER_ALL = ({("inter", "part_size", 8, ps) for ps in (0, 1, 2)} | {("inter", "part_size", S, ps) for S in (16, 32, 64) for ps in synthsyntax.INTER_PART_SIZES}
             | {("inter", "phase_luma", a, b) for a in range(4) for b in range(4)} | {("inter", "phase_chroma", a, b) for a in range(8) for b in range(8)}
             | {("inter", "gt", "on"), ("inter", "gt", "off"), ("inter", "gt_flag_on_merge"), ("inter", "gt_flag_all_zero"), ("inter", "skip"), ("inter", "root_cbf_0"),
                ("inter", "gt_pu", 4, 16), ("inter", "gt_pu", 16, 4), ("inter", "gt_pu", 8, 4), ("inter", "gt_pu", 4, 8), ("inter", "tskip", "luma"), ("inter", "tskip", "chroma")}
             | {("inter", "tr_idx", 64, t) for t in (1, 2, 3)} | {("inter", "tr_idx", 32, t) for t in range(4)} | {("inter", "tr_idx", 16, t) for t in range(3)}
             | {("inter", "mv", k) for k in ("decoded", "future", "own_cu", "margin_left", "margin_right", "margin_top", "margin_bottom", "clip")}
             | {("inter", "cbf") + t for t in itertools.product((0, 1), repeat=3)} | {("intra", "depth", d) for d in (1, 2, 3)} | LEVELS)
MIXED = {("inter", "gt", "on"), ("inter", "gt", "off"), ("inter", "mv", "decoded"), ("inter", "mv", "future"), ("inter", "mv", "own_cu"), ("intra", "depth", 3), ("inter", "depth", 3), ("inter", "tskip", "luma"), ("intra", "tskip", "luma")} | LEVELS
WANTED = {"intra_all": INTRA_ALL, "inter_all": INTER_ALL, "mixed_local": MIXED}


@pytest.mark.parametrize("name", list(synthsyntax.CASES))
def test_generated_case_holds_what_it_promises(name):
    c = synthsyntax.make_case(name)
    missing = WANTED[synthsyntax.CASES[name][0]] - c["coverage"]
    assert not missing, sorted(missing, key=str)
    # the fields outside the picture, and no level without its cbf
    W, H, parts, levels = c["W"], c["H"], c["parts"], c["levels"]
    wctu = (W + 63) // 64
    for a in range(parts.shape[0]):
        for z in range(256):
            x4, y4 = synthsyntax.zpos(z)
            if (a % wctu) * 64 + 4 * x4 >= W or (a // wctu) * 64 + 4 * y4 >= H:
                assert parts[a]["pred_mode"][z] == 15 and parts[a]["part_size"][z] == 15
                assert not levels[a, 16 * z:16 * z + 16].any() and not levels[a, 4096 + 4 * z:4096 + 4 * z + 4].any() and not levels[a, 5120 + 4 * z:5120 + 4 * z + 4].any()
    qps = (c["qp"] + 6 * (c["bd"] - 8), chroma_qp_scaled(c["qp"], c["cb_off"], c["bd"]), chroma_qp_scaled(c["qp"], c["cr_off"], c["bd"]))
    for a, z, log2cu in synthsyntax.cus(parts):
        for comp, zu, N, bit, tn in synthsyntax.cu_tus(parts[a], z, log2cu):
            base = 16 * zu if comp == 0 else (4096 if comp == 1 else 5120) + 4 * zu
            lv = levels[a, base:base + N * N]
            if (int(parts[a]["cbf"][zu][comp]) >> bit) & 1:
                assert lv.any()
                bound = synthsyntax.level_bound(c["bd"], qps[comp], N)
                assert -32768 <= lv.min() and lv.max() <= 32767 and np.abs(lv).max() <= bound
            else:
                assert not lv.any(), (a, zu, comp)
    if name == "inter_all":                                              # the clip changes some vectors, and the largest levels are the ends of the 16-bit range
        assert levels.max() == 32767 and levels.min() == -32768


@pytest.mark.parametrize("name", list(synthsyntax.CASES))
def test_generated_case_is_accepted_and_not_saturated(name):
    c = synthsyntax.make_case(name)
    lv, nl = hophip.decode_schedule(c["W"], c["H"], c["parts"], 0)      # a refusal raises
    if name == "mixed_local":
        assert nl < lv.size, (nl, lv.size)                               # multi-CTU launches are really compared
    rec, ss = reference(name)
    top = (1 << c["bd"]) - 1
    saturated = sum(int(((p == 0) | (p == top)).sum()) for p in rec)
    assert 2 * saturated < sum(p.size for p in rec), saturated
    assert (ss is None) == bool(c["plain"])


def test_chroma_qp_rule():
    """the standard's table, end to end: identity below 30, the 14 listed values, qPi - 6 above; negative values unchanged; the clip at -QpBdOffset and 57"""
    assert [chroma_qp_scaled(q, 0, 8) for q in (0, 29, 30, 34, 35, 43, 44, 51)] == [0, 29, 29, 33, 33, 37, 38, 45]
    assert chroma_qp_scaled(51, 12, 8) == 51 and chroma_qp_scaled(0, -12, 8) == 0
    assert chroma_qp_scaled(-12, -12, 10) == 0 and chroma_qp_scaled(-12, 5, 10) == 5 and chroma_qp_scaled(22, 0, 10) == 34


def test_level_bound_covers_the_16_bit_range():
    """include/hophip.h, hop_decode_frame: at every scaled QP the entry accepts, xDeQuant's product stays below 2^31 for every 16-bit level"""
    assert min(synthsyntax.level_bound(bd, q, N) for bd in (8, 10) for q in range(0, 52 + 6 * (bd - 8)) for N in (4, 8, 16, 32)) >= 32768
