"""GPU: hop_decode_frame on syntax no encoder chose (tests/synthsyntax.py) against the plain reference decoder (tests/refdecode.py, shown right on the CPU by
tests/test_refdecode_cpu.py).

The round trip of tests/test_gpu_decode.py compares the decoder with the encoder it shares its device bodies with, on what that encoder chose.  Here every generated
case -- every intra direction at every TU size, every part size on every CU size, all vector phases, GT on the smallest PUs, vectors into the sentinel, the margins and
beyond the clip, chroma QP offsets, QPs from -12 to 51, levels up to the ends of the 16-bit range -- is decoded with both schedules on a fresh context; the
reconstruction and, for the HOP configuration, the whole padded SS reference must equal the reference decoder's, sample for sample."""
import os
import sys

import numpy as np
import pytest

import synthsyntax
from hoputil import MARGIN_C, MARGIN_Y, ROOT
from test_refdecode_cpu import reference

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

pytestmark = pytest.mark.gpu


def owner(c, x, y):
    """the CU that owns luma sample (x, y): position, mode, size, transform depth, and direction or vector of the unit"""
    wctu = (c["W"] + 63) // 64
    a = (y // 64) * wctu + x // 64
    zu = synthsyntax.zidx((x & 63) >> 2, (y & 63) >> 2)
    for b, z, log2cu in synthsyntax.cus(c["parts"][a:a + 1]):
        if z <= zu < z + (1 << (2 * (log2cu - 2))):
            p = c["parts"][a][zu]
            x4, y4 = synthsyntax.zpos(z)
            where = "CU at (%d, %d) of CTU %d, %dx%d, part size %d, tr_idx %d, cbf %s, tskip %s" % ((a % wctu) * 64 + 4 * x4, (a // wctu) * 64 + 4 * y4, a, 1 << log2cu, 1 << log2cu,
                                                                                                   p["part_size"], p["tr_idx"], p["cbf"].tolist(), p["tskip"].tolist())
            if p["pred_mode"] == 1:
                return where + ", intra, luma direction %d, chroma direction %d" % (p["luma_dir"], p["chroma_dir"])
            return where + ", SS/GT, vector %s, merge %d, gt_flag %d, gt %s, skip %d" % (p["mv"].tolist(), p["merge_flag"], p["gt_flag"], p["gt"].tolist(), p["skip"])
    return "no CU"


def same(c, what, schedule, comp, got, want, margin=0):
    """exact equality; on a mismatch: plane, schedule, the first differing sample and the CU that owns it (a margin sample: the CU of the border sample it repeats)"""
    if np.array_equal(got, want):
        return
    d = np.argwhere(got != want)
    r, q = (int(v) for v in d[0])
    sh = 0 if comp == 0 else 1
    h, w = c["H"] >> sh, c["W"] >> sh
    x, y = min(max(q - margin, 0), w - 1) << sh, min(max(r - margin, 0), h - 1) << sh
    pytest.fail("%s: %s plane %d, schedule %d: %d samples differ, the first at row %d column %d (got %d, reference %d); %s"
                % (c["name"], what, comp, schedule, len(d), r - margin, q - margin, got[r, q], want[r, q], owner(c, x, y)))


def decode(ctx, c, schedule):
    ctx.decode_frame(c["parts"], c["levels"], qp=c["qp"], cb_qp_offset=c["cb_off"], cr_qp_offset=c["cr_off"], plain_intra=c["plain"], schedule=schedule)
    return [ctx.recon_download(k) for k in range(3)], (None if c["plain"] else [ctx.ssref_download(k) for k in range(3)])


@pytest.mark.parametrize("schedule", [0, 1])
@pytest.mark.parametrize("name", list(synthsyntax.CASES))
def test_decode_equals_the_reference_decoder(name, schedule):
    c = synthsyntax.make_case(name)
    want, want_ss = reference(name)
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
    try:
        got, got_ss = decode(ctx, c, schedule)
    finally:
        ctx.close()
    for k in range(3):
        same(c, "reconstruction", schedule, k, got[k], want[k])
    if not c["plain"]:
        for k, m in enumerate((MARGIN_Y, MARGIN_C, MARGIN_C)):
            same(c, "SS reference", schedule, k, got_ss[k], want_ss[k], m)


def test_second_decode_through_one_context_equals_the_first():
    """nothing is carried over from one picture to the next: inter_all twice, with another picture's SS reference and reconstruction left in between"""
    c, other = synthsyntax.make_case("inter_all"), synthsyntax.make_case("inter_all_qp51")
    ctx = hp.Context(c["W"], c["H"])
    try:
        first = decode(ctx, c, 0)
        decode(ctx, other, 0)
        second = decode(ctx, c, 0)
    finally:
        ctx.close()
    for k in range(3):
        same(c, "second reconstruction", 0, k, second[0][k], first[0][k])
        same(c, "second SS reference", 0, k, second[1][k], first[1][k], (MARGIN_Y, MARGIN_C, MARGIN_C)[k])
