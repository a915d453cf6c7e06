"""CPU: hop_slice_data_write_host -- the body of the slice-data writer (hevc-hop_amd/csrc/k_entropy_dev.inl: the syntax walk of TEncSlice::encodeSlice and the arithmetic
coder TEncBinCABAC) compiled for the host -- against the bitstreams of the UNMODIFIED reference encoder (tests/golden/slice_data.npz, tools/make_golden_slicedata.py).

Parts and levels come from the RD spine over the CPU restatement (oracle/libhop_spine_cpu.so), the coded SAO parameters from the restated loop filter and statistics with
the product's decision (tests/slicedata_cpu.py).  The slice data is the tail of the slice NAL unit's RBSP: what the writer returns must be its last sum(substream_bytes)
bytes, and the rest must be a slice header of the stored length (slicedata_util.check_header: exact for one-substream pictures, bounded by the entry points of a
wavefront picture) -- a too-short output cannot pass as a suffix.
tests/test_gpu_slicedata.py runs the device entry over the same fixture on the GPU box."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import slicedata_cpu as C
import slicedata_util as U
from hoputil import ROOT

CASES = U.slice_cases()
# the pictures coded without SAO (their slice data depends on parts and levels alone), the wavefront picture one CTU wide (no synchronisation: every row from the initial
# context models), and two of the PIC_CASES pictures with SAO: an I slice with CUs of depth 0, and the --MIsize=15 picture with partial CTUs and skipped CUs
CODED = ["64x64_raster_sao0", "192x128_wpp_sao0", "64x64_sharp77_sao0", "64x192_wpp", "136x72_plain8", "200x136_seed5_mi15"]


@pytest.fixture(scope="module")
def fixture():
    return U.load_fixture()


@pytest.mark.parametrize("key", CODED)
def test_host_writer_equals_the_reference_slice_data(fixture, key):
    c = CASES[key]
    data, sizes = C.host_slice_data(c, 0)
    assert len(sizes) == c["rows"] and int(sizes.sum()) == len(data) and np.all(sizes > 0)
    want, payload = U.fixture_slice_data(fixture, key, 0, len(data))
    assert data == want, "%s: first difference at byte %d of %d" % (key, next(i for i in range(len(data)) if data[i] != want[i]), len(data))
    U.check_header(fixture, c, 0, payload - len(data))


def test_fixture_is_tied_to_the_goldens_that_exist(fixture):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_hop_pic.json")))
    gold.update(json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_hop_pic_mi15.json"))))
    assert set(gold) <= set(CASES)
    for key, c in CASES.items():
        b = fixture[key + "/bin"].tobytes()
        assert fixture[key + "/args"].tobytes().decode() == " ".join(c["args"]), key            # the options the stream was made with are the case's
        assert len(U.slice_payloads(b)) == c["frames"], key
        if key in gold:
            assert hashlib.md5(c["input"]).hexdigest() == gold[key]["input_md5"] and hashlib.md5(b).hexdigest() == gold[key]["bin_md5"] and len(b) == gold[key]["bin_bytes"], key
    # a slice header of every one-substream configuration, a few bytes each
    for cfg in sorted(set(c["config"] for c in CASES.values() if c["rows"] == 1)):
        assert 1 <= int(fixture["header/" + cfg][0]) <= 8, cfg
    assert os.path.getsize(U.FIXTURE) < 100 * 1024


def test_coded_pictures_cover_the_syntax():
    """the parts the byte-exact test codes hold every element of the CU syntax: a weaker encoder setting cannot silently hollow the test out"""
    p = np.concatenate([C.cpu_picture(CASES[key], 0)[0].reshape(-1) for key in CODED])
    used = p["pred_mode"] != 15
    inter, intra = used & (p["pred_mode"] == 0), used & (p["pred_mode"] == 1)
    root = (p["cbf"][:, 0] | p["cbf"][:, 1] | p["cbf"][:, 2]) & 1
    share = {"depth %d" % d: (used & (p["depth"] == d)).sum() for d in range(4)}
    share.update({"SS/GT part size %d" % e: (inter & (p["part_size"] == e)).sum() for e in (0, 1, 2, 4, 5, 6, 7)})
    share.update({"transform depth %d" % t: (used & (p["tr_idx"] == t)).sum() for t in range(3)})
    share.update({"intra": intra.sum(), "intra NxN": (intra & (p["part_size"] == 3)).sum(), "skip": (inter & (p["skip"] == 1)).sum(),
                  "merge": (inter & (p["merge_flag"] == 1) & (p["skip"] == 0)).sum(), "GT": (inter & (p["gt_flag"] == 1) & (p["merge_flag"] == 0)).sum(),
                  "no GT": (inter & (p["gt_flag"] == 0) & (p["merge_flag"] == 0)).sum(), "SS/GT CU without residual": (inter & (p["skip"] == 0) & (root == 0)).sum(),
                  "transform skip": (used & (p["tskip"].sum(axis=1) > 0)).sum(), "chroma direction coded": (intra & (p["chroma_dir"] != 36)).sum()})
    assert all(v > 0 for v in share.values()), {k: int(v) for k, v in share.items() if v == 0}


def test_refusals():
    c = CASES["64x64_raster_sao0"]
    parts, levels, _ = C.cpu_picture(c, 0)
    rc, _, _, _, _ = C.write_host(c, parts, levels, None)
    assert rc == 0
    # broken parts: the validators of hop_decode_frame, and what only the syntax cares about
    for field, value in (("depth", 7), ("pred_mode", 5), ("part_size", 3), ("merge_idx", 5), ("tr_idx", 3)):
        bad = parts.copy()
        z = 0 if field != "merge_idx" else int(np.flatnonzero(bad[0]["merge_flag"] == 1)[0])
        bad[0][z][field] = value
        assert C.write_host(c, bad, levels, None)[0] == -1, field
    bad = parts.copy(); bad[0]["skip"][:16] = 1                         # a skipped CU that carries a residual or is not merged
    assert C.write_host(c, bad, levels, None)[0] == -1
    lv = levels.copy(); lv[0, 0] = 40000                                # beyond 16 bits
    assert C.write_host(c, parts, lv, None)[0] == -1
    lv = levels.copy(); lv[0, :] = 0                                    # coded blocks without a level
    assert C.write_host(c, parts, lv, None)[0] == -1
    assert C.write_host(c, parts, None, None)[0] == -1                  # the host entry has nothing resident
    # the SAO pointer and the flags disagree, either way; a parameter out of range; a merge without its candidate
    sao = np.zeros((1, 3), C.SAO_PARAM_DTYPE)
    assert C.write_host(c, parts, levels, sao)[0] == -1
    assert C.write_host(c, parts, levels, None, params=U.params_of(c, 1, 1))[0] == -1
    assert C.write_host(c, parts, levels, sao, params=U.params_of(c, 1, 1))[0] == 0
    for mode, typ, off in ((3, 0, 0), (1, 5, 0), (1, 0, 9), (2, 0, 0), (2, 1, 0)):
        s = sao.copy(); s[0, 0]["mode"] = mode; s[0, 0]["type"] = typ; s[0, 0]["offset"][0] = off
        assert C.write_host(c, parts, levels, s, params=U.params_of(c, 1, 1))[0] == -1, (mode, typ, off)
    # parameters
    for name, value in (("slice_type", 5), ("slice_type", 2), ("wpp", 2), ("qp", 52), ("plain_intra", 1)):
        p = U.params_of(c); setattr(p, name, value)
        assert C.write_host(c, parts, levels, None, params=p)[0] == -1, name


@pytest.mark.parametrize("key", ["64x64_raster_sao0", "192x128_wpp_sao0"])
def test_capacity_is_a_hard_bound(key):
    """out_capacity one byte short: an error, the needed size in n_substreams' place, and not one byte stored behind the buffer"""
    c = CASES[key]
    parts, levels, _ = C.cpu_picture(c, 0)
    data, sizes = C.host_slice_data(c, 0)
    rc, buf, guard, got, nsub = C.write_host(c, parts, levels, None, capacity=len(data) - 1, guard=64)
    assert rc == -1 and nsub == len(data) and np.all(guard == 0xA5)
    assert np.array_equal(got[:len(sizes)], sizes)                      # the true sizes all the same
    rc, buf, guard, got, nsub = C.write_host(c, parts, levels, None, capacity=len(data), guard=64)
    assert rc == 0 and nsub == c["rows"] and buf.tobytes() == data and np.all(guard == 0xA5)
    rc, _, guard, _, nsub = C.write_host(c, parts, levels, None, capacity=0, guard=64)
    assert rc == -1 and nsub == len(data) and np.all(guard == 0xA5)
