"""CPU: the reference encoder's streams at QP 22 / 27 / 37 (tests/golden/stream_qps.npz, tools/make_golden_qps.py) through the host yardsticks.  Every other reference
stream of the repository is coded at QP 32 (or the 10-bit plain case's 27): this pins reader, parser, writer, decoder, both loop filters and the CPU spine at QPs they
were never held to the reference encoder at -- four different qp % 6, both sides of the chroma QP table's knee at 30 -- before tests/test_gpu_picture_qps.py leans on
the same streams for the pictures of a stack coded side by side at different QPs.  No device is touched."""
import ctypes
import hashlib

import numpy as np
import pytest

import picture_qps_util as Q
import stream_read_util as R
import stream_util as S
from hoputil import oracle, oracle_deblock
from refdecode import ref_decode

IDS = ["%s_q%d" % s for s in Q.STREAMS]
_read = {}


def read(key, qp):
    """hop_access_unit_read_host of the stream: (info, rbsp, sizes, digest), once"""
    if (key, qp) not in _read:
        _read[(key, qp)] = R.hophip().access_unit_read_host(Q.stream(key, qp), None)
    return _read[(key, qp)]


def slice_fields(info):
    s = info.params.slice
    return (s.slice_type, s.wpp, s.plain_intra, s.sao_luma, s.sao_chroma, s.mi_size)


def test_the_fixture_holds_what_the_tests_lean_on():
    """per case: pairwise different slice data that shrinks as the QP rises, one pair of SAO flags"""
    for key, qps in Q.QPS.items():
        data = [read(key, qp)[1] for qp in qps]
        assert len(set(data)) == len(qps), key
        assert all(len(a) > len(b) for a, b in zip(data[:-1], data[1:])), (key, [len(d) for d in data])
        assert len({slice_fields(read(key, qp)[0])[3:5] for qp in qps}) == 1, key


@pytest.mark.parametrize("key,qp", Q.STREAMS, ids=IDS)
def test_reader_finds_the_coded_qp(key, qp):
    c = Q.CASES[key]
    info, rbsp, sizes, digest = read(key, qp)
    want = read(key, 32)[0]
    assert info.params.slice.qp == qp
    assert slice_fields(info) == slice_fields(want)                           # every other slice field is the QP-32 stream's
    assert (info.pic_w, info.pic_h, info.bit_depth, info.n_substreams) == (c["W"], c["H"], c["bd"], c["rows"])
    assert (info.params.poc, info.params.parameter_sets, info.params.hash, info.nal_type) == (0, 1, 1, 19)
    assert len(sizes) == c["rows"] and int(sizes.sum()) == len(rbsp)


@pytest.mark.parametrize("key,qp", Q.STREAMS, ids=IDS)
def test_parse_then_write_gives_the_input_back(key, qp):
    hp = R.hophip()
    info, rbsp, sizes, _ = read(key, qp)
    kw = R.parse_kwargs(info)
    parts, levels, sao = hp.slice_data_parse_host(info.pic_w, info.pic_h, rbsp, sizes, **kw)
    data, got_sizes, nsub = hp.slice_data_write_host(info.pic_w, info.pic_h, parts, levels, sao, **kw)
    assert nsub == len(sizes) and np.array_equal(got_sizes[:nsub], sizes) and data == rbsp, (key, qp)
    if qp != 32:                                                              # the models of another QP do not read these bytes: an error, or other syntax
        try:
            other = hp.slice_data_parse_host(info.pic_w, info.pic_h, rbsp, sizes, **dict(kw, qp=32))
            assert other[0].tobytes() != parts.tobytes() or not np.array_equal(other[1], levels), (key, qp)
        except hp.HopError as e:
            assert e.code == -1


@pytest.mark.parametrize("key,qp", Q.STREAMS, ids=IDS)
def test_decoded_picture_is_the_one_the_sei_names(key, qp):
    """the reference decoder of tests/refdecode.py over the parsed parts and levels, the oracle's deblocking filter, the parsed SAO parameters resolved by
    hop_sao_reconstruct_params and applied by the oracle's offsetting pass: the MD5 of every plane is the one in the stream's SEI"""
    hp = R.hophip()
    c = Q.CASES[key]
    info, rbsp, sizes, digest = read(key, qp)
    W, H, bd = info.pic_w, info.pic_h, info.bit_depth
    parts, levels, sao = hp.slice_data_parse_host(W, H, rbsp, sizes, **R.parse_kwargs(info))
    rec, _ = ref_decode(W, H, parts, levels, qp, 0, 0, bd, 1 if c["plain"] else 0)
    final = oracle_deblock(W, H, (qp, 0, 0, 0, 0), parts, rec, bd)
    assert sao is not None
    recon = hp.sao_reconstruct_params(sao, (W + 63) // 64, bd)
    O = oracle()
    P3 = ctypes.c_void_p * 3
    final = [np.ascontiguousarray(a, np.int16) for a in final]
    out = [np.zeros_like(a) for a in final]
    O.hop_o_sao_apply.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    assert O.hop_o_sao_apply(W, H, bd, P3(*[a.ctypes.data for a in final]), recon.ctypes.data_as(ctypes.c_void_p), P3(*[a.ctypes.data for a in out])) == 0
    for comp in range(3):
        assert bytes(digest[comp]) == hashlib.md5(out[comp].astype(np.uint8).tobytes()).digest(), (key, qp, comp)


@pytest.mark.parametrize("qp", (22, 37))
def test_cpu_spine_writes_the_reference_stream(qp):
    """hop_spine_cpu_encode_wpp at the QP, the oracle's loop filters with the product's SAO decision (stream_util.cpu_final_picture), hop_access_unit_write_host: the
    reference encoder's .bin byte for byte"""
    c = Q.case_at("192x128_wpp", qp)
    parts, levels, sao, rec = S.cpu_final_picture(c, 0)
    rc, au, n, _ = S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 1))
    want = Q.stream("192x128_wpp", qp)
    assert rc == 0 and n == len(au)
    assert au == want, S.first_difference(au, want)
