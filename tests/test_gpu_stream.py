"""GPU: hop_access_unit_write, hop_rbsp_escape, hop_picture_hash (csrc/k_stream.hip) -- the outer layer of the stream from the device.

The escape launches (count / scan / scatter) against the host entry and the sequential restatement on crafted buffers; the checksum pass and the MD5 of uploaded planes
against numpy and hashlib; whole access units, byte for byte, against the bitstreams of the UNMODIFIED reference encoder (tests/golden/slice_data.npz "<key>/bin",
tests/golden/stream_hash.npz) and against the host entry on the downloaded levels and reconstruction."""
import hashlib

import numpy as np
import pytest

import slicedata_util as U
import stream_util as S
from hoputil import lenslet

pytestmark = pytest.mark.gpu

CASES = U.slice_cases()
STREAM_CASES = ("64x64_raster", "64x192_wpp", "128x64_2frames", "136x72_plain10", "64x64_raster_sao0", "192x128_seed7_mi15_wpp")
_hp = None


def hophip():
    global _hp
    if _hp is None:
        import importlib.util, os
        spec = importlib.util.spec_from_file_location("hophip", os.path.join(U.ROOT, "hevc-hop_amd", "hophip.py"))
        _hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(_hp)
    return _hp


@pytest.fixture(scope="module")
def small_ctx():
    ctx = hophip().Context(64, 64)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", S.ESCAPE_LENGTHS)
def test_device_escape_equals_host_and_restatement(small_ctx, n):
    hp = hophip()
    for name, a in S.escape_contents(n).items():
        data = a.tobytes()
        want, _ = S.escape_restated(data)
        for seg in S.escape_segmentations(a, n):
            got, cnt = small_ctx.rbsp_escape(data, seg, guard=64)
            host, host_cnt = hp.rbsp_escape_host(data, seg, lib=small_ctx.L)
            assert got == want, "%d %s %s: %s" % (n, name, seg, S.first_difference(got, want))
            assert host == want and np.array_equal(cnt, host_cnt), (n, name, seg, cnt, host_cnt)
            at = 0
            for k, s in enumerate(seg):
                assert cnt[k] == S.escape_restated(data[at:at + s])[1], (n, name, seg, k)
                at += s
    # one byte short: the guard bytes behind the buffer stay untouched (asserted in the binding), the size needed is reported
    data = S.escape_contents(n)["zeros"].tobytes()
    want, _ = S.escape_restated(data)
    with pytest.raises(hp.HopError) as e:
        small_ctx.rbsp_escape(data, None, capacity=len(want) - 1, guard=64)
    assert e.value.code == -1 and e.value.needed == len(want)
    assert small_ctx.rbsp_escape(data, None, capacity=len(want), guard=64)[0] == want


def test_device_escape_refuses_empty_segments(small_ctx):
    hp = hophip()
    for seg in ([2, 0], [0]):
        with pytest.raises(hp.HopError) as e:
            small_ctx.rbsp_escape(b"\x01\x02"[:sum(seg)], seg)
        assert e.value.code == -1
    with pytest.raises(hp.HopError):
        small_ctx.rbsp_escape(b"", [])
    assert small_ctx.rbsp_escape(b"\x00\x00\x01", None)[0] == b"\x00\x00\x03\x01"      # and the context stays usable


def checksum_numpy(plane, bd):
    h, w = plane.shape
    y, x = np.mgrid[0:h, 0:w]
    m = ((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff
    v = plane.astype(np.int64) & 0xffff
    s = ((v & 0xff) ^ m).sum()
    if bd > 8:
        s += ((v >> 8) ^ m).sum()
    return int(s) & 0xffffffff


@pytest.mark.parametrize("bd", (8, 10))
def test_picture_hash_of_uploaded_planes(bd):
    hp = hophip()
    W, H = 264, 16                                                           # wider than 256: x >> 8 counts
    ctx = hp.Context(W, H, bit_depth=bd)
    rng = np.random.RandomState(bd)
    top = (1 << bd) - 1
    for kind in ("random", "zero", "max"):
        planes = []
        for comp in range(3):
            shape = (H, W) if comp == 0 else (H // 2, W // 2)
            a = rng.randint(0, top + 1, shape).astype(np.int16) if kind == "random" else np.full(shape, 0 if kind == "zero" else top, np.int16)
            ctx.plane_upload("recon", comp, a); planes.append(a)
        sums, md5 = ctx.picture_hash(3), ctx.picture_hash(1)
        for comp, a in enumerate(planes):
            want = checksum_numpy(a, bd)
            assert bytes(sums[0, comp]) == want.to_bytes(4, "big") + bytes(12), (bd, kind, comp, bytes(sums[0, comp]).hex(), hex(want))
            raw = a.astype(np.uint8).tobytes() if bd == 8 else a.astype("<u2").tobytes()
            assert bytes(md5[0, comp]) == hashlib.md5(raw).digest(), (bd, kind, comp)
    with pytest.raises(hp.HopError):
        ctx.picture_hash(2)
    ctx.close()


def stream_args(c):
    return dict(qp=c["qp"], slice_type=c["slice_type"], wpp=c["wpp"], plain_intra=1 if c["plain"] else 0, mi_size=c["mi"])


def code_and_filter(ctx, c, planes):
    """one picture through the context up to its final reconstruction: (parts, coded SAO parameters or None)"""
    ctx.upload_orig(*planes)
    parts = ctx.encode_frame(c["qp"], c["mi"], 0, None, wpp=c["wpp"], wavefront_lag=5 if c["wpp"] else 0, plain_intra=1 if c["plain"] else 0)[3]
    ctx.deblock_frame(parts, c["qp"])
    sao = ctx.sao_frame(U.sao_lambdas(c["qp"]), c["slice_type"], c["qp"], int(ctx.rd_fraction_download()[-1]), enabled=(1, 1, 1)) if c["sao"] else None
    return parts, sao


@pytest.mark.parametrize("key", STREAM_CASES)
def test_device_stream_equals_the_reference_encoder(key):
    hp = hophip()
    c = CASES[key]
    want = U.load_fixture()[key + "/bin"].tobytes()
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], slots=0 if c["plain"] else 16)
    got = b""
    for k, planes in enumerate(c["pictures"]):                              # (the context reused for a second picture)
        parts, sao = code_and_filter(ctx, c, planes)
        au, sizes = ctx.access_unit_write(parts, None, sao, poc=k, parameter_sets=1 if k == 0 else 0, hash=1, guard=256, **stream_args(c))
        assert len(sizes) == 1 and int(sizes[0]) == len(au)
        rec = [ctx.recon_download(comp) for comp in range(3)]
        host = hp.access_unit_write_host(c["W"], c["H"], parts, ctx.levels_download(), sao, rec, bit_depth=c["bd"], poc=k, parameter_sets=1 if k == 0 else 0, hash=1,
                                         lib=ctx.L, **stream_args(c))
        assert au == host, "%s picture %d, device against host: %s" % (key, k, S.first_difference(au, host))
        got += au
        if key in S.HASH_CASES and c["plain"] is None:                      # the checksum hash, from the device pass
            sum_want = np.load(S.HASH_FIXTURE)[key + "/bin"].tobytes()
            sum_got = ctx.access_unit_write(parts, None, sao, poc=0, parameter_sets=1, hash=3, **stream_args(c))[0]
            assert sum_got == sum_want, "%s checksum: %s" % (key, S.first_difference(sum_got, sum_want))
    ctx.close()
    assert got == want, "%s: %s" % (key, S.first_difference(got, want))


def test_stacked_pictures_equal_the_pictures_alone():
    """three 192x128 pictures in one stacked context: each au_bytes[p] slice is the access unit of the picture written alone"""
    hp = hophip()
    c = CASES["192x128_wpp_sao0"]
    pics = [lenslet(192, 128, 16, seed) for seed in (7, 21, 22)]
    st = hp.Context(192, 128, pictures=3, slots=16)
    st.upload_orig(st.stack([p[0] for p in pics]), st.stack([p[1] for p in pics], True), st.stack([p[2] for p in pics], True))
    parts = st.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=5)[3]
    st.deblock_frame(parts, 32)
    data, sizes = st.access_unit_write(parts, None, None, hash=1, guard=256, **stream_args(c))
    summed = st.access_unit_write(parts, None, None, hash=3, **stream_args(c))[0]
    st.close()
    assert len(sizes) == 3 and int(sizes.sum()) == len(data)
    one = hp.Context(192, 128, slots=16)
    at = 0
    for k, planes in enumerate(pics):
        p1, _ = code_and_filter(one, c, planes)
        alone = one.access_unit_write(p1, None, None, hash=1, **stream_args(c))[0]
        assert data[at:at + int(sizes[k])] == alone, "picture %d: %s" % (k, S.first_difference(data[at:at + int(sizes[k])], alone))
        if k == 2:
            alone3 = one.access_unit_write(p1, None, None, hash=3, **stream_args(c))[0]
            assert summed.endswith(alone3)
        at += int(sizes[k])
    one.close()


def test_state_and_capacity():
    hp = hophip()
    c = CASES["64x64_raster_sao0"]
    ctx = hp.Context(64, 64, slots=16)
    parts, _ = code_and_filter(ctx, c, c["pictures"][0])
    want = ctx.access_unit_write(parts, None, None, hash=1, **stream_args(c))[0]
    for cap in (len(want) - 1, 100, 0):                                    # one byte short; not even the slice data; none
        with pytest.raises(hp.HopError) as e:
            ctx.access_unit_write(parts, None, None, hash=1, capacity=cap, guard=256, **stream_args(c))
        assert e.value.code == -1 and e.value.needed == len(want), (cap, e.value.needed, len(want))
    assert ctx.access_unit_write(parts, None, None, hash=1, capacity=len(want), guard=256, **stream_args(c))[0] == want
    with pytest.raises(hp.HopError) as e:
        ctx.access_unit_write(parts, None, None, hash=2, **stream_args(c))
    assert e.value.code == -1
    # hop_decode_frame keeps no levels: a NULL call is refused with HOP_ERR_STATE, the levels handed in are coded, the context stays usable
    lv = ctx.levels_download()
    ctx.decode_frame(parts, lv, qp=32)
    ctx.deblock_frame(parts, 32)
    with pytest.raises(hp.HopError) as e:
        ctx.access_unit_write(parts, None, None, hash=1, **stream_args(c))
    assert e.value.code == -3
    assert ctx.access_unit_write(parts, lv, None, hash=1, **stream_args(c))[0] == want
    ctx.close()
