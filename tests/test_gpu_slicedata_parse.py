"""GPU: hop_slice_data_parse -- the slice data of a picture parsed on the device (csrc/k_parse.hip: one wave per substream, the rows of a wavefront picture in diagonal
launches) -- on the slice data of the UNMODIFIED reference encoder's streams (tests/golden/slice_data.npz).

Every picture is coded once per module: hop_upload_orig -> hop_encode_frame -> hop_deblock_frame -> hop_sao_frame -> hop_slice_data_write, keeping parts, levels, the
coded SAO parameters, the reconstruction before and after the loop filters and the SS reference.  Then, per case: the fixture's bytes parse to the encoder's data (the
comparison and the one mask rule of tests/test_slicedata_parse_cpu.py); the device entry and the host build agree; the parsed data decodes to the encoder's pictures;
parse, then write, gives the bytes back.  All comparisons are exact."""

import numpy as np
import pytest

import slicedata_parse_util as P
import slicedata_util as U
from hoputil import lenslet

pytestmark = pytest.mark.gpu

CASES = U.slice_cases()
KEYS = ["64x64_sharp77", "192x128_wpp", "64x192_wpp", "128x256_wpp", "200x136_seed5_mi15", "192x128_seed7_mi15_wpp", "136x72_plain10", "128x64_2frames",
        "448x192_seed3_mi15_wpp"]
_done = {}


def planes(ctx):
    return [ctx.recon_download(c) for c in range(3)]


def code_picture(ctx, c, pl):
    """one picture through the encoder's context: what a decoder has to reproduce, and the writer's bytes"""
    ctx.upload_orig(*pl)
    parts = ctx.encode_frame(c["qp"], c["mi"], 0, None, wpp=c["wpp"], wavefront_lag=5 if c["wpp"] else 0, plain_intra=1 if c["plain"] else 0)[3]
    r = {"parts": parts, "levels": ctx.levels_download(), "recon": planes(ctx), "ssref": None if c["plain"] else [ctx.ssref_download(k) for k in range(3)], "sao": None}
    if c["sao"]:
        ctx.deblock_frame(parts, c["qp"])
        r["sao"] = ctx.sao_frame(U.sao_lambdas(c["qp"]), c["slice_type"], c["qp"], int(ctx.rd_fraction_download()[-1]), enabled=(1, 1, 1))
        r["final"] = planes(ctx)
    r["data"], r["sizes"], r["nsub"] = ctx.slice_data_write(parts, None, r["sao"], c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, mi_size=c["mi"])
    return r


def coded(key):
    """every picture of the case coded once, and parsed once from the FIXTURE's bytes by the device entry and by the host build"""
    if key not in _done:
        hp = P.hophip()
        c = CASES[key]
        G = U.load_fixture()
        ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], slots=0 if c["plain"] else 16)
        out = []
        for k, pl in enumerate(c["pictures"]):
            r = code_picture(ctx, c, pl)
            r["fixture"] = U.fixture_slice_data(G, key, k, len(r["data"]))[0]
            r["parsed"] = ctx.slice_data_parse(r["fixture"], r["sizes"], **P.parse_kwargs(c))
            r["host"] = hp.slice_data_parse_host(c["W"], c["H"], r["fixture"], r["sizes"], bit_depth=c["bd"], lib=ctx.L, **P.parse_kwargs(c))
            out.append(r)
        ctx.close()
        _done[key] = out
    return _done[key]


@pytest.mark.parametrize("key", KEYS)
def test_parsed_equals_the_encoders_data(key):
    for k, r in enumerate(coded(key)):
        assert r["fixture"] == r["data"], (key, k)                          # (the writer's bytes are the reference's: tests/test_gpu_slicedata.py)
        parts, levels, sao = r["parsed"]
        assert np.array_equal(levels, r["levels"]), (key, k)
        assert (sao is None) == (r["sao"] is None) and (sao is None or sao.tobytes() == r["sao"].tobytes()), (key, k)
        P.assert_parts_equal(parts, r["parts"], "%s picture %d" % (key, k))


@pytest.mark.parametrize("key", KEYS)
def test_device_and_host_entries_agree(key):
    for k, r in enumerate(coded(key)):
        for got, want in zip(r["parsed"], r["host"]):
            assert (got is None) == (want is None) and (got is None or got.tobytes() == want.tobytes()), (key, k)


@pytest.mark.parametrize("key", KEYS)
def test_bitstream_to_picture(key):
    """hop_decode_frame on the parsed parts and levels gives the encoder's reconstruction before the loop filters and its SS reference; hop_deblock_frame,
    hop_sao_reconstruct_params on the parsed SAO parameters and hop_sao_apply then give its final picture"""
    hp = P.hophip()
    c = CASES[key]
    d = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
    for k, r in enumerate(coded(key)):
        parts, levels, sao = r["parsed"]
        d.decode_frame(parts, levels, qp=c["qp"], plain_intra=1 if c["plain"] else 0)
        for comp, (got, want) in enumerate(zip(planes(d), r["recon"])):
            assert np.array_equal(got, want), (key, k, comp)
        if r["ssref"] is not None:
            for comp in range(3):
                assert np.array_equal(d.ssref_download(comp), r["ssref"][comp]), (key, k, "ssref", comp)
        if sao is not None:
            d.deblock_frame(parts, c["qp"])
            d.sao_apply(d.sao_reconstruct_params(sao))
            for comp, (got, want) in enumerate(zip(planes(d), r["final"])):
                assert np.array_equal(got, want), (key, k, "final", comp)
    d.close()


@pytest.mark.parametrize("key", KEYS)
def test_parse_then_write_gives_the_input_back(key):
    hp = P.hophip()
    c = CASES[key]
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
    for k, r in enumerate(coded(key)):
        parts, levels, sao = r["parsed"]
        data, sizes, nsub = ctx.slice_data_write(parts, levels, sao, c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, mi_size=c["mi"])
        assert data == r["fixture"] and np.array_equal(sizes, r["sizes"]) and nsub == c["rows"], (key, k)
    ctx.close()


def test_stacked_pictures_equal_the_pictures_alone():
    """three 192x128 pictures in one stacked context, written and parsed as a stack: each picture's data is that of the picture parsed alone"""
    hp = P.hophip()
    c = CASES["192x128_wpp_sao0"]
    kw = P.parse_kwargs(c)
    pics = [lenslet(192, 128, 16, seed) for seed in (7, 21, 22)]
    st = hp.Context(192, 128, pictures=3, slots=16)
    st.upload_orig(st.stack([p[0] for p in pics]), st.stack([p[1] for p in pics], True), st.stack([p[2] for p in pics], True))
    parts = st.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=5)[3]
    levels = st.levels_download()
    data, sizes, nsub = st.slice_data_write(parts, None, None, 32, 3, 1, 0)
    assert nsub == 2 and len(sizes) == 6
    got = st.slice_data_parse(data, sizes, **kw)
    st.close()
    assert got[2] is None and np.array_equal(got[1], levels)
    P.assert_parts_equal(got[0], parts, "stack")
    one = hp.Context(192, 128)
    at = 0
    for k in range(3):
        n = int(sizes[2 * k:2 * k + 2].sum())
        alone = one.slice_data_parse(data[at:at + n], sizes[2 * k:2 * k + 2], **kw)
        assert alone[0].tobytes() == got[0][6 * k:6 * k + 6].tobytes() and np.array_equal(alone[1], got[1][6 * k:6 * k + 6]), k
        at += n
    one.close()
    assert at == len(data)


def test_errors_leave_the_context_usable():
    hp = P.hophip()
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("shard", os.path.join(U.ROOT, "hevc-hop_amd", "shard.py"))
    shard = importlib.util.module_from_spec(spec); spec.loader.exec_module(shard)
    c = CASES["192x128_wpp_sao0"]
    kw = P.parse_kwargs(c)
    ctx = hp.Context(c["W"], c["H"], slots=16)
    r = code_picture(ctx, c, c["pictures"][0])
    right = ctx.slice_data_parse(r["data"], r["sizes"], **kw)
    P.assert_parts_equal(right[0], r["parts"], "192x128_wpp_sao0")
    # refused before anything is enqueued: a wrong n_substreams, a zero size, a sharded context
    for over, sizes in (({"n_substreams": 1}, r["sizes"]), ({"n_substreams": 3}, r["sizes"]), ({}, np.array([0, len(r["data"])], np.uint32))):
        with pytest.raises(hp.HopError) as e:
            ctx.slice_data_parse(r["data"], sizes, **P.parse_kwargs(c, **over))
        assert e.value.code == -1
    class Dummy:
        fn = shard.ALLGATHER_FN(lambda user, send, recv, nbytes: 0)
    dummy = Dummy()
    ctx.set_shard(0, 2, dummy)
    with pytest.raises(hp.HopError) as e:
        ctx.slice_data_parse(r["data"], r["sizes"], **kw)
    assert e.value.code == -1 and "sharded" in str(e.value)
    ctx.set_shard(0, 1, None)
    # found on the device: the last substream cut by four bytes (the host build under the sanitizers handles this input cleanly: tools/slicedata_parse_check.cpp's
    # tails and tests/test_slicedata_parse_cpu.py) -- HOP_ERR_ARG naming the substream; the host build agrees
    cut = r["sizes"].copy(); cut[-1] -= 4
    with pytest.raises(hp.HopError) as e:
        ctx.slice_data_parse(r["data"][:-4], cut, **kw)
    assert e.value.code == -1 and "substream 1" in str(e.value), str(e.value)
    with pytest.raises(hp.HopError) as h:
        hp.slice_data_parse_host(c["W"], c["H"], r["data"][:-4], cut, lib=ctx.L, **kw)
    for got, want in zip(e.value.outputs, h.value.outputs):
        assert (got is None) == (want is None) and (got is None or got.tobytes() == want.tobytes())
    again = ctx.slice_data_parse(r["data"], r["sizes"], **kw)                # and a correct call on the same context afterwards
    assert again[0].tobytes() == right[0].tobytes() and np.array_equal(again[1], right[1])
    data, sizes, nsub = ctx.slice_data_write(r["parts"], None, None, 32, 3, 1, 0)   # the resident levels of hop_encode_frame are untouched
    assert data == r["data"]
    ctx.close()
