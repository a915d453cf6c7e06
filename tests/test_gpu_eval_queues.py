"""GPU: the evaluation chains of hop_encode_frame on S streams (HOP_SPINE_STREAMS) out of K buffer sets (HOP_SPINE_SETS), placed by expected length (hop_eval_place):
whatever S and K are, the encode computes the same bytes.  The picture is the smallest committed one where a round holds more than four groups and more than one CTU row
is in flight: 448x192, seed 3, --MIsize=15, WaveFrontSynchro, lag-5 wavefront, 48 candidate slots (a CU's first sub-CU evaluated with it) -- 21 CTUs, against the
reference encoder's run (tests/golden/encoder_spine_mi15.npz).  The library reads both switches per call."""
import os
import tempfile

import numpy as np
import pytest

from hoputil import ROOT
from hoputil import lenslet
from test_spine_cpu import check_against_golden, key_mi15

pytestmark = pytest.mark.gpu

W, H, SEED, LAG, SLOTS = 448, 192, 3, 5, 48


def _hp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def encode():
    """one encode of the picture under the switches set at the moment: checked against the golden; returns (reconstruction planes, levels, stats)"""
    hp = _hp()
    G = np.load(os.path.join(ROOT, "tests", "golden", "encoder_spine_mi15.npz"))
    Y, Cb, Cr = lenslet(W, H, 15, SEED)
    ctx = hp.Context(W, H, slots=SLOTS)
    ctx.upload_orig(Y, Cb, Cr)
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "t.txt")
        cost, bits, dist, parts, nc = ctx.encode_frame(32, 15, 0, tp, wpp=1, wavefront_lag=LAG)
        text = open(tp, "rb").read()
    check_against_golden(G, key_mi15(W, H, SEED, LAG), cost, bits, dist, parts.view(np.dtype(parts.dtype.descr)), text)
    rec = [ctx.recon_download(c).copy() for c in range(3)]
    levels = ctx.levels_download().copy()
    stats = ctx.encode_stats()
    ctx.close()
    print({k: stats[k] for k in ("evaluation_wait", "evaluation_handover", "intra_cu", "inter_cu", "inter_cu_skip")})
    return rec, levels, stats


@pytest.fixture(scope="module")
def default_run():
    """the run with neither switch set (computed once, left unchanged)"""
    saved = {k: os.environ.pop(k) for k in ("HOP_SPINE_STREAMS", "HOP_SPINE_SETS") if k in os.environ}
    try:
        return encode()
    finally:
        os.environ.update(saved)


def test_default_streams_and_sets_no_group_waits_for_a_buffer(default_run):
    rec, levels, stats = default_run
    assert stats["evaluation_handover"]["calls"] == 0
    assert stats["evaluation_wait"]["calls"] > 0


@pytest.mark.parametrize("streams", [1, 2, 8])
def test_any_number_of_streams_computes_the_same_bytes(streams, default_run, monkeypatch):
    monkeypatch.delenv("HOP_SPINE_SETS", raising=False)
    monkeypatch.setenv("HOP_SPINE_STREAMS", str(streams))
    rec, levels, stats = encode()
    for c in range(3):
        assert rec[c].tobytes() == default_run[0][c].tobytes(), c
    assert levels.tobytes() == default_run[1].tobytes()
    assert (stats["evaluation_wait"]["calls"] > 0) == (streams > 1)      # one stream: no evaluation streams at all


def test_two_buffer_sets_take_the_hand_over_path(default_run, monkeypatch):
    monkeypatch.delenv("HOP_SPINE_STREAMS", raising=False)
    monkeypatch.setenv("HOP_SPINE_SETS", "2")
    rec, levels, stats = encode()
    for c in range(3):
        assert rec[c].tobytes() == default_run[0][c].tobytes(), c
    assert levels.tobytes() == default_run[1].tobytes()
    assert stats["evaluation_handover"]["calls"] > 0
