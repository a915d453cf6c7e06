"""CPU: hop_slice_data_parse_host -- the body of the slice-data parser (hevc-hop_amd/csrc/k_parse_dev.inl: the CTU loop of TDecSlice::decompressSlice, the TDecSbac parsers,
the arithmetic decoder TDecBinCABAC and the derivations of a decoder) compiled for the host -- on the slice data of the UNMODIFIED reference encoder's streams
(tests/golden/slice_data.npz).

The input is the fixture's bytes, not the writer's; the expected parts, levels and SAO parameters come from the CPU path (tests/slicedata_cpu.py).  All comparisons are
exact.  One field is masked, on some units (slicedata_parse_util.masked): gt_flag on the units of an SS / GT CU that are not a PU's first unit -- the stream carries one
flag per PU.  tests/test_slicedata_cpu.py::test_coded_pictures_cover_the_syntax asserts that the six pictures hold every element of the CU syntax.
tests/test_gpu_slicedata_parse.py runs the device entry on the GPU box; tools/slicedata_parse_check.cpp runs the same damaged streams under ASan / UBSan."""
import ctypes

import numpy as np
import pytest

import slicedata_cpu as C
import slicedata_parse_util as P
import slicedata_util as U
from test_slicedata_cpu import CODED

CASES = U.slice_cases()


@pytest.fixture(scope="module")
def fixture():
    return U.load_fixture()


_in = {}


def stream(fixture, key):
    """the reference encoder's slice data of the case's first picture and its substream sizes"""
    if key not in _in:
        data, sizes = C.host_slice_data(CASES[key], 0)
        want, _ = U.fixture_slice_data(fixture, key, 0, len(data))
        _in[key] = (want, sizes)
    return _in[key]


def parse(c, data, sizes, **over):
    return P.hophip().slice_data_parse_host(c["W"], c["H"], data, sizes, bit_depth=c["bd"], lib=C.hophip_host(), **P.parse_kwargs(c, **over))


@pytest.mark.parametrize("key", CODED)
def test_parsed_equals_the_encoders_data(fixture, key):
    c = CASES[key]
    data, sizes = stream(fixture, key)
    want_parts, want_levels, want_sao = C.cpu_picture(c, 0)
    parts, levels, sao = parse(c, data, sizes)
    assert np.array_equal(levels, want_levels), key                         # all 6144 per CTU
    assert (sao is None) == (want_sao is None) and (sao is None or sao.tobytes() == want_sao.tobytes()), key
    P.assert_parts_equal(parts, want_parts, key)
    only_parts = parse(c, data, sizes, want_levels=False)                    # levels == NULL: parts and SAO alone
    assert only_parts[1] is None and only_parts[0].tobytes() == parts.tobytes()


@pytest.mark.parametrize("key", CODED)
def test_parse_then_write_gives_the_input_back(fixture, key):
    c = CASES[key]
    data, sizes = stream(fixture, key)
    parts, levels, sao = parse(c, data, sizes)
    rc, buf, _, got_sizes, nsub = C.write_host(c, parts, levels, sao)
    assert rc == 0 and nsub == c["rows"] and np.array_equal(got_sizes[:nsub], sizes) and buf[:len(data)].tobytes() == data, key


def test_mi_size_is_read(fixture):
    """the micro-image candidates of the merge and AMVP lists depend on mi_size: the same bytes parsed with 16 instead of 15 give other vectors"""
    key = "200x136_seed5_mi15"
    c = CASES[key]
    data, sizes = stream(fixture, key)
    right = parse(c, data, sizes)[0]
    try:
        other = parse(c, data, sizes, mi_size=16)[0]
    except P.hophip().HopError as e:                                        # other vectors may make other contexts: the stream may stop making sense
        other = e.outputs[0]
    assert np.any(other["mv"] != right["mv"])


def test_refusals():
    c = CASES["192x128_wpp_sao0"]
    hp = P.hophip()
    data, sizes = C.host_slice_data(c, 0)
    assert parse(c, data, sizes)[0].shape == (6, 256)
    for over in ({"n_substreams": 1}, {"n_substreams": 3}, {"sao_luma": 1, "sao_chroma": 1, "n_substreams": 2},       # (the binding allocates sao_coded by the flags)
                 {"slice_type": 5}, {"slice_type": 2}, {"wpp": 2}, {"qp": 52}, {"plain_intra": 1}, {"mi_size": 0}, {"mi_size": -1}):
        with pytest.raises(hp.HopError) as e:
            if "sao_luma" in over:
                raw_parse(c, data, sizes, P.parse_kwargs(c, sao_luma=1, sao_chroma=1), with_sao=False)
            else:
                parse(c, data, sizes, **over)
        assert e.value.code == -1, over
    with pytest.raises(hp.HopError) as e:                                   # a zero size (the other substream takes the bytes: the sum still fits the data)
        parse(c, data, np.array([0, len(data)], np.uint32))
    assert e.value.code == -1
    raw = CASES["64x64_raster_sao0"]
    d1, s1 = C.host_slice_data(raw, 0)
    with pytest.raises(hp.HopError):
        parse(raw, d1, s1, n_substreams=2)
    with pytest.raises(hp.HopError):                                        # sao_coded without an SAO flag
        raw_parse(raw, d1, s1, P.parse_kwargs(raw), with_sao=True)


def raw_parse(c, data, sizes, kw, with_sao):
    """hop_slice_data_parse_host with sao_coded given or not whatever the flags say"""
    hp = P.hophip()
    n = C.cpu_picture(c, 0)[0].shape[0]
    p = U.SliceDataParams(kw["qp"], kw["slice_type"], kw["wpp"], kw["plain_intra"], kw["sao_luma"], kw["sao_chroma"], kw["mi_size"])
    buf = np.frombuffer(data, np.uint8).copy(); sizes = np.ascontiguousarray(sizes, np.uint32)
    parts = np.zeros((n, 256), hp.CU_PART_DTYPE); levels = np.zeros((n, 6144), np.int32); sao = np.zeros((n, 3), hp.SAO_PARAM_DTYPE)
    L = C.hophip_host()
    L.hop_slice_data_parse_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_void_p] * 3
    r = L.hop_slice_data_parse_host(c["W"], c["H"], c["bd"], ctypes.byref(p), buf.ctypes.data, sizes.ctypes.data, len(sizes), parts.ctypes.data, levels.ctypes.data,
                                    sao.ctypes.data if with_sao else None)
    if r:
        e = hp.HopError("hop_slice_data_parse_host: %d" % r); e.code = r
        raise e


@pytest.mark.parametrize("key", ["64x64_raster_sao0", "192x128_wpp_sao0", "136x72_plain8"])
def test_a_stream_cut_short_is_an_error(fixture, key):
    """the last byte gone, and the size says so: the decoder runs past the end or finds no stop pattern -- HOP_ERR_ARG, and the guards behind the outputs untouched (the
    binding asserts them)"""
    c = CASES[key]
    data, sizes = stream(fixture, key)
    cut = sizes.copy(); cut[-1] -= 1
    with pytest.raises(P.hophip().HopError) as e:
        parse(c, data[:-1], cut)
    assert e.value.code == -1


@pytest.mark.parametrize("key", CODED)
def test_damaged_streams_end_in_ok_or_an_error(fixture, key):
    """100 seeded variants per picture (slicedata_parse_util.variants; tools/slicedata_parse_check.cpp runs the same under the sanitizers): each returns HOP_OK or
    HOP_ERR_ARG with the guards untouched, and what it returned as HOP_OK is partition data hop_decode_schedule accepts or refuses -- nothing else"""
    c = CASES[key]
    hp = P.hophip()
    data, sizes = stream(fixture, key)
    ok = 0
    for i, kind, d, s in P.variants(data, sizes, P.case_seed(c["W"], c["H"])):
        try:
            parts = parse(c, d, s)[0]
        except hp.HopError as e:
            assert e.code == -1, (key, i, kind)
            continue
        ok += 1
        try:
            hp.decode_schedule(c["W"], c["H"], parts, lib=C.hophip_host())
        except hp.HopError as e:
            assert "-1" in str(e), (key, i, kind)
    assert 0 <= ok <= 100
