"""GPU: hop_rbsp_unescape, hop_access_unit_read, hop_access_unit_decode (csrc/k_stream.hip) -- the stream read back on the device.

The unescape launches (count / scan / compact) against the host entry and the Python restatement of the position rule; the device reader against the host reader on every
fixture access unit and the crafted ones; and the strongest check the project has: a context that never saw an original decodes the bytes of the UNMODIFIED reference
encoder (tests/golden/slice_data.npz "<key>/bin", tests/golden/stream_hash.npz) and reproduces the hash the reference put into the stream for its own reconstruction."""
import hashlib

import numpy as np
import pytest

import slicedata_util as U
import stream_read_util as R
import stream_util as S

pytestmark = pytest.mark.gpu

CASES = R.CASES
STREAMS = R.streams()
DECODE_CASES = ("64x64_raster", "64x192_wpp", "128x256_wpp", "128x64_2frames", "136x72_plain10", "64x64_sharp77", "192x128_seed7_mi15_wpp", "448x192_seed3_mi15_wpp")


@pytest.fixture(scope="module")
def small_ctx():
    ctx = R.hophip().Context(64, 64)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", S.ESCAPE_LENGTHS)
def test_device_unescape_equals_host_and_restatement(small_ctx, n):
    hp = R.hophip()
    for name, a in S.escape_contents(n).items():
        data = a.tobytes()
        esc = S.escape_restated(data)[0]
        if data[-1] == 0:
            esc = esc[:-1]
        for seg in R.escaped_segmentations(esc):                            # (both boundary cuts: in front of and behind an inserted 03)
            got, sizes, viol = small_ctx.rbsp_unescape(esc, seg, guard=64)
            host, host_sizes, host_viol = hp.rbsp_unescape_host(esc, seg, lib=small_ctx.L)
            want, want_sizes, want_viol = R.position_rule(esc, 0, seg)
            assert got == data == host == want, "%d %s %s: %s" % (n, name, seg, S.first_difference(got, want))
            assert sizes.tolist() == host_sizes.tolist() == want_sizes and viol == host_viol == want_viol == 0, (n, name, seg, sizes.tolist(), want_sizes, viol)
        # the same bytes taken as they are (not escaped): violations and removals wherever the content has them, and two bytes of lookback
        if n > 2:
            for back in (0, 2):
                got, sizes, viol = small_ctx.rbsp_unescape(data, [n - back], lookback=back, guard=64)
                want, want_sizes, want_viol = R.position_rule(data, back, [n - back])
                assert (got, sizes.tolist(), viol) == (want, want_sizes, want_viol), (n, name, back, viol, want_viol)
                assert hp.rbsp_unescape_host(data, [n - back], lookback=back, lib=small_ctx.L)[2] == want_viol
    # one byte short of capacity: the size needed is reported, the guard stays intact (asserted in the binding), the context stays usable
    esc = S.escape_restated(S.escape_contents(n)["001"].tobytes())[0]
    want = R.position_rule(esc, 0, [len(esc)])[0]
    with pytest.raises(hp.HopError) as e:
        small_ctx.rbsp_unescape(esc, None, capacity=len(want) - 1, guard=64)
    assert e.value.code == -1 and e.value.needed == len(want)
    assert small_ctx.rbsp_unescape(esc, None, capacity=len(want), guard=64)[0] == want


def test_device_unescape_crafted_and_refusals(small_ctx):
    hp = R.hophip()
    assert small_ctx.rbsp_unescape(b"\x00\x00\x02")[::2] == (b"\x00\x00\x02", 1)
    assert small_ctx.rbsp_unescape(b"\x00\x00\x03\x04")[::2] == (b"\x00\x00\x04", 1)
    assert small_ctx.rbsp_unescape(b"\x05\x00\x00\x03\x01", [3, 2])[1].tolist() == [3, 1]
    assert small_ctx.rbsp_unescape(b"\x05\x00\x00\x03\x01", [4, 1])[1].tolist() == [3, 1]
    assert small_ctx.rbsp_unescape(b"\x00\x00\x03\x01", None, lookback=2)[0] == b"\x01"
    for data, seg, back in ((b"\x01\x02", [2, 0], 0), (b"", [], 0), (b"\x01\x02\x03\x04", [1], 3)):
        with pytest.raises(hp.HopError) as e:
            small_ctx.rbsp_unescape(data, seg, lookback=back)
        assert e.value.code == -1
    assert small_ctx.rbsp_unescape(b"\x00\x00\x03\x01")[0] == b"\x00\x00\x01"


def same_read(a, b):
    return bytes(a[0]) == bytes(b[0]) and a[1] == b[1] and a[2].tolist() == b[2].tolist() and np.array_equal(a[3], b[3])


def test_device_reader_equals_the_host_reader():
    hp = R.hophip()
    ctxs = {}
    n_read = 0
    units = [(key, CASES[key]["W"], CASES[key]["H"], CASES[key]["bd"], hp.annexb_access_units(stream)) for _, key, stream, _ in STREAMS]
    units += [(name, 64, 64 * len(subs), 8, [au]) for name, au, subs in R.crafted()]
    for name, W, H, bd, aus in units:
        ctx = ctxs.get((W, H, bd)) or ctxs.setdefault((W, H, bd), hp.Context(W, H, bit_depth=bd))
        active = None
        for k, au in enumerate(aus):
            host = hp.access_unit_read_host(au, active, lib=ctx.L)
            dev = ctx.access_unit_read(au, active)
            assert same_read(dev, host), (name, k)
            active = active or host[0]
            n_read += 1
    # refusals of the device entry: another picture size, a violation, too little room -- and the context reads on
    ctx = ctxs[(64, 64, 8)]
    good = [au for name, au, subs in R.crafted() if name == "drawn_1"][0]
    for bad in ([au for name, au, subs in R.crafted() if name == "drawn_3"][0], R.access_unit(64, 64, R.slice_nal(None, 0, offsets=[], raw_payload=b"\x41\x00\x00\x02\x80"), 0)):
        with pytest.raises(hp.HopError) as e:
            ctx.access_unit_read(bad)
        assert e.value.code == -1
    with pytest.raises(hp.HopError) as e:
        ctx.access_unit_read(good, capacity=599)
    assert e.value.code == -1 and e.value.needed == 600
    assert same_read(ctx.access_unit_read(good), hp.access_unit_read_host(good, lib=ctx.L))
    stack = hp.Context(64, 64, pictures=2)
    with pytest.raises(hp.HopError) as e:
        stack.access_unit_read(good)
    assert e.value.code == -1
    stack.close()
    for c in ctxs.values():
        c.close()
    assert n_read == 20 + len(R.crafted())


def checksum_numpy(plane, bd):
    """calcChecksum (TComPicYuvMD5.cpp:141-164) restated, as in tests/test_gpu_stream.py"""
    h, w = plane.shape
    y, x = np.mgrid[0:h, 0:w]
    m = ((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff
    v = plane.astype(np.int64) & 0xffff
    s = ((v & 0xff) ^ m).sum()
    if bd > 8:
        s += ((v >> 8) ^ m).sum()
    return int(s) & 0xffffffff


def decode_stream(ctx, hp, stream, method, bd):
    """every access unit of a reference stream through hop_access_unit_decode; checks the hash both ways and the side outputs against the parser on the reader's RBSP"""
    active = None
    for k, au in enumerate(hp.annexb_access_units(stream)):
        info, match, parts, levels, sao = ctx.access_unit_decode(au, active)
        assert match == [1, 1, 1], (k, match)
        rinfo, rbsp, sizes, digest = ctx.access_unit_read(au, active)
        assert bytes(rinfo) == bytes(info) and info.params.hash == method
        planes = [ctx.recon_download(comp) for comp in range(3)]            # (the parse below leaves the picture alone)
        for comp, a in enumerate(planes):
            if method == 1:
                raw = a.astype(np.uint8).tobytes() if bd == 8 else a.astype("<u2").tobytes()
                assert hashlib.md5(raw).digest() == bytes(digest[comp]), (k, comp)
            else:
                assert checksum_numpy(a, bd).to_bytes(4, "big") + bytes(12) == bytes(digest[comp]), (k, comp)
        kw = {n: v for n, v in R.parse_kwargs(info).items() if n != "bit_depth"}
        p2, l2, s2 = ctx.slice_data_parse(rbsp, sizes, **kw)
        assert parts.tobytes() == p2.tobytes() and np.array_equal(levels, l2) and (sao is None) == (s2 is None) and (sao is None or sao.tobytes() == s2.tobytes()), k
        active = active or info


@pytest.mark.parametrize("key", DECODE_CASES)
def test_stream_to_picture(key):
    hp = R.hophip()
    c = CASES[key]
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])                     # no original is ever uploaded
    decode_stream(ctx, hp, U.load_fixture()[key + "/bin"].tobytes(), 1, c["bd"])
    ctx.close()


@pytest.mark.parametrize("key", S.HASH_CASES)
def test_checksum_stream_to_picture(key):
    hp = R.hophip()
    c = CASES[key]
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
    decode_stream(ctx, hp, np.load(S.HASH_FIXTURE)[key + "/bin"].tobytes(), 3, c["bd"])
    ctx.close()


def test_failure_paths():
    hp = R.hophip()
    c = CASES["192x128_wpp"]
    au = hp.annexb_access_units(U.load_fixture()["192x128_wpp/bin"].tobytes())[0]
    ctx = hp.Context(c["W"], c["H"])
    info = ctx.access_unit_decode(au, want_outputs=False)[0]
    # one digest byte flipped in the SEI (no emulation prevention inside this one: the three MD5s are the 48 bytes in front of the trailing byte): that plane alone
    # stops matching
    sei = S.split_units(au)[-1][1]
    assert S.split_units(au)[-1][2] == 40 and b"\x00\x00\x03" not in sei[3:] and len(sei) == 3 + 2 + 3 + 48 + 1
    for plane in range(3):
        first = len(au) - 1 - 48 + 16 * plane
        at = next(i for i in range(first + 2, first + 14) if 0 not in au[i - 2:i + 3] and au[i] != 0x10)   # (the flip must not create emulation prevention)
        bad = au[:at] + bytes([au[at] ^ 0x10]) + au[at + 1:]
        match = ctx.access_unit_decode(bad, want_outputs=False)[1]
        assert match == [0 if k == plane else 1 for k in range(3)], (plane, match)
        assert ctx.access_unit_decode(au, want_outputs=False)[1] == [1, 1, 1]
    # one slice-data byte flipped: a parse error naming the substream, or a picture that does not match
    vcl_at = [p + len(u) - len(u.lstrip(b"\x00")) + 1 for p, u, t in S.split_units(au) if t < 32][0]
    for off in (40, 500):
        at = vcl_at + info.header_bytes + off
        bad = au[:at] + bytes([au[at] ^ 0x55]) + au[at + 1:]
        try:
            match = ctx.access_unit_decode(bad, want_outputs=False)[1]
            assert match != [1, 1, 1], off
        except hp.HopError as e:
            assert e.code == -1 and ("substream" in str(e) or "emulation prevention" in str(e)), e
        assert ctx.access_unit_decode(au, want_outputs=False)[1] == [1, 1, 1]
    ctx.close()


def test_round_trip_on_the_device():
    """encode 192x128_wpp_sao0, write its access unit, decode those bytes in a second context: the encoder's final planes, all hashes matching"""
    hp = R.hophip()
    c = CASES["192x128_wpp_sao0"]
    enc = hp.Context(c["W"], c["H"], slots=16)
    enc.upload_orig(*c["pictures"][0])
    parts = enc.encode_frame(c["qp"], c["mi"], 0, None, wpp=1, wavefront_lag=5)[3]
    enc.deblock_frame(parts, c["qp"])
    want = [enc.recon_download(comp) for comp in range(3)]
    au = enc.access_unit_write(parts, None, None, qp=c["qp"], slice_type=3, wpp=1, plain_intra=0, mi_size=c["mi"], hash=1)[0]
    levels = enc.levels_download()
    enc.close()
    dec = hp.Context(c["W"], c["H"])
    info, match, p2, l2, sao = dec.access_unit_decode(au)
    assert match == [1, 1, 1] and sao is None and np.array_equal(l2, levels)
    for comp in range(3):
        assert np.array_equal(dec.recon_download(comp), want[comp]), comp
    dec.close()
