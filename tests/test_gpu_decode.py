"""GPU: hop_decode_frame -- a picture reconstructed from its syntax alone on a context that never saw the original.

The encoder (hop_encode_frame, pinned to the reference by tests/test_gpu_spine.py) codes a golden picture; its parts and levels go to a fresh context, whose decode
must leave the encoder context's reconstruction before the loop filters and its whole padded SS reference, sample for sample, with either schedule; then the loop
filters (deblocking, SAO from the coded parameters through hop_sao_reconstruct_params) must give the same final picture."""
import os
import sys

import numpy as np
import pytest

from hoputil import ROOT, lenslet, sao_cases
from test_spine_cpu import FRAMES, FRAMES_MI15, frame

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip as hp  # noqa: E402

pytestmark = pytest.mark.gpu


def planes(ctx):
    return [ctx.recon_download(c) for c in range(3)]


def ssref(ctx):
    return [ctx.ssref_download(c) for c in range(3)]


def encode(W, H, Y, Cb, Cr, bd=8, qp=32, mi=16, lag=0, plain=0, slots=0):
    e = hp.Context(W, H, bit_depth=bd, slots=slots)                 # (candidate slots change the encoder's speed, not its result)
    e.upload_orig(Y, Cb, Cr)
    parts = e.encode_frame(qp, mi, 0, None, wpp=1 if lag else 0, wavefront_lag=lag, plain_intra=plain)[3]
    return e, parts, e.levels_download()


def check_roundtrip(W, H, Y, Cb, Cr, bd=8, qp=32, mi=16, lag=0, plain=0, filters=True, slots=0):
    e, parts, levels = encode(W, H, Y, Cb, Cr, bd, qp, mi, lag, plain, slots)
    want = planes(e)
    want_ss = ssref(e) if not plain else None
    d = hp.Context(W, H, bit_depth=bd)
    for schedule in (1, 0):
        d.decode_frame(parts, levels, qp=qp, plain_intra=plain, schedule=schedule)
        got = planes(d)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (schedule, c, np.argwhere(got[c] != want[c])[:5])
        if want_ss is not None:
            for c, s in enumerate(ssref(d)):
                assert np.array_equal(s, want_ss[c]), (schedule, "ssref", c, np.argwhere(s != want_ss[c])[:5])
    if filters:                                                       # deblocking, then SAO: the encoder's coded parameters, the decoder's reconstruction of them
        for ctx in (e, d):
            ctx.deblock_frame(parts, qp)
        for c in range(3):
            assert np.array_equal(planes(d)[c], planes(e)[c]), ("deblocked", c)
        lam = 0.57 * 2.0 ** ((qp - 12) / 3.0)
        coded = e.sao_frame([lam, lam, lam], 2 if plain else 3, qp, int(e.rd_fraction_download()[-1]))
        d.sao_apply(d.sao_reconstruct_params(coded))
        for c in range(3):
            assert np.array_equal(planes(d)[c], planes(e)[c]), ("sao", c)
    e.close(); d.close()
    return parts


@pytest.mark.parametrize("W,H,seed,sharp", FRAMES)
def test_decode_equals_encode(W, H, seed, sharp):
    Y, Cb, Cr = frame(W, H, seed, sharp)
    check_roundtrip(W, H, Y, Cb, Cr)


def test_decode_equals_encode_wavefront():
    Y, Cb, Cr = lenslet(448, 192, 16, 3)
    parts = check_roundtrip(448, 192, Y, Cb, Cr, lag=5)
    lv, nl = hp.decode_schedule(448, 192, parts, 0)
    assert nl < lv.size


@pytest.mark.parametrize("W,H,seed,lag", FRAMES_MI15)
def test_decode_equals_encode_mi15(W, H, seed, lag):
    Y, Cb, Cr = lenslet(W, H, 15, seed)
    check_roundtrip(W, H, Y, Cb, Cr, mi=15, lag=lag or 0)


@pytest.mark.parametrize("bd,qp", [(8, 32), (10, 22), (10, 37)])
def test_decode_plain_intra(bd, qp):
    Y, Cb, Cr = lenslet(136, 72, 16, 9)
    if bd > 8:
        rng = np.random.RandomState(9)
        Y, Cb, Cr = (np.clip(p.astype(np.int32) * 4 + rng.randint(0, 4, p.shape), 0, 1023).astype(np.int16) for p in (Y, Cb, Cr))
    check_roundtrip(136, 72, Y, Cb, Cr, bd=bd, qp=qp, plain=1)


@pytest.mark.parametrize("case", sao_cases(), ids=lambda c: "%s_%dx%d_%dbit" % (c["key"], c["W"], c["H"], c["bd"]))
def test_sao_reconstruct_params_apply_gives_the_reference_output(case):
    W, H = case["W"], case["H"]
    ctx = hp.Context(W, H, bit_depth=case["bd"])
    for c in range(3):
        a = np.ascontiguousarray(case["in"][c], np.int16)
        ctx._chk(ctx.L.hop_recon_upload(ctx.h, c, a.ctypes.data), "hop_recon_upload")
    ctx.sao_apply(ctx.sao_reconstruct_params(case["coded"].view(hp.SAO_PARAM_DTYPE)))
    for c in range(3):
        assert np.array_equal(ctx.recon_download(c), case["out"][c]), c
    ctx.close()


def test_two_pictures_through_one_context():
    """the second decode starts from the sentinel: it must not see the first picture's SS reference"""
    W, H = 128, 64
    d = hp.Context(W, H)
    for seed in (11, 12):
        Y, Cb, Cr = lenslet(W, H, 16, seed)
        e, parts, levels = encode(W, H, Y, Cb, Cr)
        d.decode_frame(parts, levels, qp=32)
        for c in range(3):
            assert np.array_equal(d.recon_download(c), e.recon_download(c)), (seed, c)
            assert np.array_equal(d.ssref_download(c), e.ssref_download(c)), (seed, c)
        e.close()
    d.close()


def test_bench_geometry_decode_equals_encode():
    """the bench frame's geometry: 7728 wide, --MIsize=15, lag 8 (8 CTU rows)"""
    Y, Cb, Cr = lenslet(7728, 512, 15, 2)
    check_roundtrip(7728, 512, Y, Cb, Cr, mi=15, lag=8, filters=False, slots=48)


def test_refusals_enqueue_nothing():
    W, H = 128, 64
    Y, Cb, Cr = lenslet(W, H, 16, 11)
    e, parts, levels = encode(W, H, Y, Cb, Cr)
    d = hp.Context(W, H)
    d.decode_frame(parts, levels, qp=32)
    before = ssref(d) + planes(d)
    bad = parts.copy(); bad[0]["luma_dir"][:] = 40; bad[0]["pred_mode"][:] = 1; bad[0]["part_size"][:] = 0
    with pytest.raises(hp.HopError):
        d.decode_frame(bad, levels, qp=32)
    with pytest.raises(hp.HopError):
        d.decode_frame(parts, levels, qp=32, schedule=3)
    after = ssref(d) + planes(d)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    s = hp.Context(W, H, pictures=2)
    with pytest.raises(hp.HopError):
        s.decode_frame(np.concatenate([parts, parts]), np.concatenate([levels, levels]), qp=32)
    s.close(); e.close(); d.close()
