"""GPU: hop_slice_data_write -- the slice data of a picture written on the device (csrc/k_entropy.hip: a context pass and a coding pass, one wave per substream) -- byte
for byte against the bitstreams of the UNMODIFIED reference encoder (tests/golden/slice_data.npz, tools/make_golden_slicedata.py).

Every fixture case goes hop_upload_orig -> hop_encode_frame -> hop_deblock_frame -> hop_sao_frame -> hop_slice_data_write(levels = NULL: the resident levels); the cases
coded without SAO skip the loop filters and pass no SAO parameters.  WaveFrontSynchro cases run as the wavefront.  What comes back must be the tail of the slice NAL
unit's RBSP and leave a slice header of the stored length in front (slicedata_util.check_header: exact for one-substream pictures, bounded by the entry points otherwise).  The host build of the same body (hop_slice_data_write_host, on
the downloaded levels) must give the same bytes and sizes."""
import numpy as np
import pytest

import slicedata_util as U
from hoputil import lenslet

pytestmark = pytest.mark.gpu

CASES = U.slice_cases()
_done = {}


def hophip():
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(U.ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def code_picture(hp, ctx, c, planes):
    """one picture through the context: (parts, coded SAO parameters or None, slice data, substream sizes, n_substreams)"""
    ctx.upload_orig(*planes)
    parts = ctx.encode_frame(c["qp"], c["mi"], 0, None, wpp=c["wpp"], wavefront_lag=5 if c["wpp"] else 0, plain_intra=1 if c["plain"] else 0)[3]
    sao = None
    if c["sao"]:
        ctx.deblock_frame(parts, c["qp"])
        sao = ctx.sao_frame(U.sao_lambdas(c["qp"]), c["slice_type"], c["qp"], int(ctx.rd_fraction_download()[-1]), enabled=(1, 1, 1))
    data, sizes, nsub = ctx.slice_data_write(parts, None, sao, c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, mi_size=c["mi"])
    return parts, sao, data, sizes, nsub


def coded(key):
    """every picture of the case coded once: a list of dicts (device output, the host entry's output on the downloaded levels)"""
    if key not in _done:
        hp = hophip()
        c = CASES[key]
        ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], slots=0 if c["plain"] else 16)
        out = []
        for planes in c["pictures"]:                                        # (the context and its buffers reused for a second picture)
            parts, sao, data, sizes, nsub = code_picture(hp, ctx, c, planes)
            host = hp.slice_data_write_host(c["W"], c["H"], parts, ctx.levels_download(), sao, c["bd"], c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, mi_size=c["mi"], lib=ctx.L)
            out.append({"data": data, "sizes": sizes, "nsub": nsub, "host": host})
        ctx.close()
        _done[key] = out
    return _done[key]


@pytest.fixture(scope="module")
def fixture():
    return U.load_fixture()


@pytest.mark.parametrize("key", list(CASES))
def test_device_writer_equals_the_reference_slice_data(fixture, key):
    c = CASES[key]
    for k, r in enumerate(coded(key)):
        assert r["nsub"] == c["rows"] == len(r["sizes"]) and int(r["sizes"].sum()) == len(r["data"]) and np.all(r["sizes"] > 0), (key, k)
        want, payload = U.fixture_slice_data(fixture, key, k, len(r["data"]))
        assert r["data"] == want, "%s picture %d: first difference at byte %d of %d" % (key, k, next(i for i in range(len(want)) if r["data"][i] != want[i]), len(want))
        U.check_header(fixture, c, k, payload - len(r["data"]))


@pytest.mark.parametrize("key", list(CASES))
def test_device_and_host_entries_agree(key):
    for r in coded(key):
        data, sizes, nsub = r["host"]
        assert nsub == r["nsub"] and np.array_equal(sizes, r["sizes"]) and data == r["data"], key


def test_stacked_pictures_equal_the_pictures_alone():
    """three 192x128 pictures in one stacked context, coded as one wavefront: each picture's substreams are those of the picture coded alone"""
    hp = hophip()
    c = CASES["192x128_wpp_sao0"]
    pics = [lenslet(192, 128, 16, seed) for seed in (7, 21, 22)]
    st = hp.Context(192, 128, pictures=3, slots=16)
    st.upload_orig(st.stack([p[0] for p in pics]), st.stack([p[1] for p in pics], True), st.stack([p[2] for p in pics], True))
    parts = st.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=5)[3]
    data, sizes, nsub = st.slice_data_write(parts, None, None, 32, 3, 1, 0)
    assert nsub == 2 and len(sizes) == 6
    host_levels = st.levels_download()
    again = st.slice_data_write(parts, host_levels, None, 32, 3, 1, 0)   # and the same from levels handed in
    assert again[0] == data and np.array_equal(again[1], sizes)
    st.close()
    at = 0
    one = hp.Context(192, 128, slots=16)
    for k, planes in enumerate(pics):
        alone = coded("192x128_wpp_sao0")[0] if k == 0 else dict(zip(("data", "sizes", "nsub"), code_picture(hp, one, c, planes)[2:]))
        n = int(sizes[2 * k:2 * k + 2].sum())
        assert np.array_equal(sizes[2 * k:2 * k + 2], alone["sizes"]) and data[at:at + n] == alone["data"], k
        at += n
    one.close()
    assert at == len(data)


def test_short_capacity_is_refused_and_the_context_stays_usable():
    hp = hophip()
    c = CASES["192x128_wpp_sao0"]
    want = coded("192x128_wpp_sao0")[0]
    ctx = hp.Context(c["W"], c["H"], slots=16)
    ctx.upload_orig(*c["pictures"][0])
    parts = ctx.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=5)[3]
    for cap in (len(want["data"]) - 1, int(want["sizes"][0]), 0):          # one byte short; room for the first substream only; none
        with pytest.raises(hp.HopError) as e:
            ctx.slice_data_write(parts, None, None, 32, 3, 1, 0, capacity=cap, guard=256)    # (the binding asserts the guard bytes behind the buffer untouched)
        assert e.value.code == -1 and e.value.needed == len(want["data"]) and str(len(want["data"])) in str(e.value)
    data, sizes, nsub = ctx.slice_data_write(parts, None, None, 32, 3, 1, 0, capacity=len(want["data"]), guard=256)     # exactly enough
    assert data == want["data"] and np.array_equal(sizes, want["sizes"]) and nsub == 2
    # the other refusals, before anything is enqueued: SAO pointer and flags disagreeing, broken parts, nothing resident
    with pytest.raises(hp.HopError): ctx.slice_data_write(parts, None, None, 32, 3, 1, 0, sao_luma=1, sao_chroma=1)
    bad = parts.copy(); bad[0][0]["depth"] = 7
    with pytest.raises(hp.HopError): ctx.slice_data_write(bad, None, None, 32, 3, 1, 0)
    # hop_decode_frame keeps no levels: after it the resident ones belong to no picture the context holds -- a NULL call is refused, the levels handed in are coded
    lv = ctx.levels_download()
    ctx.decode_frame(parts, lv, qp=32)
    with pytest.raises(hp.HopError) as e: ctx.slice_data_write(parts, None, None, 32, 3, 1, 0)
    assert e.value.code == -3
    assert ctx.slice_data_write(parts, lv, None, 32, 3, 1, 0)[0] == want["data"]
    ctx.close()
    fresh = hp.Context(c["W"], c["H"])
    with pytest.raises(hp.HopError) as e: fresh.slice_data_write(parts, None, None, 32, 3, 1, 0)
    assert e.value.code == -3                                              # HOP_ERR_STATE
    fresh.close()
