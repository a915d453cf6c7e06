"""CPU: the stream read back (host/hop_stream_read.cpp) -- hop_annexb_access_unit, hop_access_unit_read_host, hop_rbsp_unescape_host -- on the WHOLE bitstreams of the
unmodified reference encoder (tests/golden/slice_data.npz "<key>/bin", tests/golden/stream_hash.npz), on crafted access units around a Python restatement of the slice
header, and on damaged bytes.  What the reader returns goes straight into hop_slice_data_parse_host, which refuses a substream whose consumed length differs from its
size: that pins the entry-point arithmetic on every stream without an encoder run.  No device is touched."""
import ctypes
import hashlib

import numpy as np
import pytest

import slicedata_util as U
import stream_read_util as R
import stream_util as S
from slicedata_cpu import cpu_affordable

CASES = R.CASES
STREAMS = R.streams()
AFFORDABLE = [k for k, c in CASES.items() if cpu_affordable(c)]


def read_all(hp, stream):
    """[(access unit, info, rbsp, sizes, digest)] of a whole stream, the first picture's info as `active` of the later ones"""
    out, active = [], None
    for au in hp.annexb_access_units(stream):
        info, rbsp, sizes, digest = hp.access_unit_read_host(au, active)
        active = active or info
        out.append((au, info, rbsp, sizes, digest))
    return out


@pytest.mark.parametrize("name,key,stream,method", STREAMS, ids=[s[0] for s in STREAMS])
def test_fixture_streams(name, key, stream, method):
    hp = R.hophip()
    c = CASES[key]
    G = U.load_fixture()
    got = read_all(hp, stream)
    assert len(got) == c["frames"] and b"".join(g[0] for g in got) == stream
    payloads = U.slice_payloads(stream)
    for k, (au, info, rbsp, sizes, digest) in enumerate(got):
        s = info.params.slice
        assert (info.pic_w, info.pic_h, info.bit_depth, s.qp, s.slice_type, s.wpp, s.plain_intra, s.sao_luma, s.sao_chroma) == \
               (c["W"], c["H"], c["bd"], c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, c["sao"], c["sao"]), (name, k)
        assert s.mi_size == (0 if c["plain"] else c["mi"])
        assert (info.params.poc, info.params.parameter_sets, info.params.hash) == (k, 1 if k == 0 else 0, method)
        assert info.n_substreams == c["rows"] == len(sizes) and int(sizes.sum()) == len(rbsp)
        assert info.nal_type == (19 if k == 0 else 1 if c["plain"] else 0)
        assert len(rbsp) > 0 and payloads[k].endswith(rbsp), (name, k)
        U.check_header(G, c, k, len(payloads[k]) - len(rbsp))
        # the escaped header: the two bytes of the NAL unit header, the RBSP header, and the 03s inside it
        vcl = [u for u in U.nal_units(au) if ((u[0] >> 1) & 0x3F) < 32][0]
        assert U.strip_emulation_prevention(vcl[:info.header_bytes])[2:] == payloads[k][:len(payloads[k]) - len(rbsp)]
        hp.slice_data_parse_host(info.pic_w, info.pic_h, rbsp, sizes, want_levels=False, **R.parse_kwargs(info))                              # HopError unless HOP_OK
        assert digest[:, 4 if method == 3 else 16:].sum() == 0 and digest.any(axis=1).all()


@pytest.mark.parametrize("key", AFFORDABLE)
def test_reader_against_the_writer(key):
    """RBSP and sizes are hop_slice_data_write_host's, the digest is the MD5 of the CPU path's final picture, and the recovered params write the access unit back"""
    hp = R.hophip()
    c = CASES[key]
    for k, (au, info, rbsp, sizes, digest) in enumerate(read_all(hp, U.load_fixture()[key + "/bin"].tobytes())):
        parts, levels, sao, rec = S.cpu_final_picture(c, k)
        data, want_sizes, _ = hp.slice_data_write_host(c["W"], c["H"], parts, levels, sao, bit_depth=c["bd"], **{n: v for n, v in R.parse_kwargs(info).items() if n != "bit_depth"})
        assert rbsp == data and np.array_equal(sizes, want_sizes), (key, k)
        for comp in range(3):
            raw = rec[comp].astype(np.uint8).tobytes() if c["bd"] == 8 else rec[comp].astype("<u2").tobytes()
            assert bytes(digest[comp]) == hashlib.md5(raw).digest(), (key, k, comp)
        rc, again, n, _ = S.access_unit_host(c, parts, levels, sao, rec, S.StreamParams.from_buffer_copy(bytes(info.params)))
        assert rc == 0 and again == au, "%s picture %d: %s" % (key, k, S.first_difference(again, au))


@pytest.mark.parametrize("n", S.ESCAPE_LENGTHS)
def test_host_unescape_against_the_restatement(n):
    hp = R.hophip()
    for name, a in S.escape_contents(n).items():
        data = a.tobytes()
        esc, _ = S.escape_restated(data)
        if data[-1] == 0:
            esc = esc[:-1]                                                  # (the final 03 behind a trailing 00 is no emulation prevention byte unless two zeros precede it)
        for seg in R.escaped_segmentations(esc):
            got, sizes, viol = hp.rbsp_unescape_host(esc, seg, guard=64)
            want, want_sizes, want_viol = R.position_rule(esc, 0, seg)
            assert got == data == want, (n, name, seg)
            assert sizes.tolist() == want_sizes and int(sizes.sum()) == len(got), (n, name, seg, sizes.tolist(), want_sizes)
            assert viol == want_viol == 0, (n, name, seg, viol)
    # one byte short: nothing behind the capacity is touched (asserted in the binding), the size needed is reported
    esc = S.escape_restated(S.escape_contents(n)["001"].tobytes())[0]
    want = R.position_rule(esc, 0, [len(esc)])[0]
    with pytest.raises(hp.HopError) as e:
        hp.rbsp_unescape_host(esc, None, capacity=len(want) - 1, guard=64)
    assert e.value.code == -1 and e.value.needed == len(want)
    assert hp.rbsp_unescape_host(esc, None, capacity=len(want), guard=64)[0] == want


def test_unescape_violations_lookback_and_refusals():
    hp = R.hophip()
    assert hp.rbsp_unescape_host(b"\x00\x00\x02")[::2] == (b"\x00\x00\x02", 1)
    assert hp.rbsp_unescape_host(b"\x00\x00\x03\x04")[::2] == (b"\x00\x00\x04", 1)
    assert hp.rbsp_unescape_host(b"\x00\x00\x03\x03")[::2] == (b"\x00\x00\x03", 0)
    assert hp.rbsp_unescape_host(b"\x00\x00\x00\x00")[2] == 2
    # the bytes in front of the first segment feed the predicate and are not output
    for back, data, want in ((2, b"\x00\x00\x03\x01", b"\x01"), (1, b"\x00\x00\x03\x01", b"\x00\x01"), (1, b"\x00\x03\x01", b"\x03\x01"), (2, b"\x07\x00\x00\x03\x01", b"\x00\x01")):
        got, sizes, viol = hp.rbsp_unescape_host(data, None, lookback=back)
        assert (got, sizes.tolist(), viol) == (want, [len(want)], 0) == R.position_rule(data, back, [len(data) - back])[:1] + ([len(want)], 0), (back, data)
    # an 03 exactly at a boundary belongs to the segment that starts there
    assert hp.rbsp_unescape_host(b"\x05\x00\x00\x03\x01", [3, 2])[1].tolist() == [3, 1]
    assert hp.rbsp_unescape_host(b"\x05\x00\x00\x03\x01", [4, 1])[1].tolist() == [3, 1]
    for data, seg, back in ((b"\x01\x02", [2, 0], 0), (b"", [], 0), (b"\x01\x02\x03\x04", [1], 3), (b"", [1], -1)):   # an empty segment, none, a lookback outside 0..2
        with pytest.raises(hp.HopError) as e:
            hp.rbsp_unescape_host(data, seg, lookback=back)
        assert e.value.code == -1


CRAFTED = R.crafted()


@pytest.mark.parametrize("name,au,subs", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted_access_units(name, au, subs):
    hp = R.hophip()
    info, rbsp, sizes, digest = hp.access_unit_read_host(au)
    assert rbsp == b"".join(subs) and sizes.tolist() == [len(s) for s in subs], (name, sizes.tolist())
    assert info.n_substreams == len(subs) and info.params.hash == 0 and not digest.any()
    vcl = [u for u in U.nal_units(au) if ((u[0] >> 1) & 0x3F) < 32][0]
    head = U.strip_emulation_prevention(vcl[:info.header_bytes])
    assert U.strip_emulation_prevention(vcl) == head + rbsp
    if name == "header_03":
        assert info.header_bytes > len(head)                                # the header itself holds emulation prevention bytes
    if name.startswith("boundary"):
        assert sizes.tolist() == [4, 3, 1]


def ok_or_refused(hp, au, active=None):
    try:
        hp.access_unit_read_host(au, active, capacity=len(au))              # (the binding asserts the 0xA5 guard bytes behind all four outputs)
        return 0
    except hp.HopError as e:
        assert e.code == -1, e
        return -1


def test_every_prefix_is_read_or_refused():
    hp = R.hophip()
    stream = U.load_fixture()["64x64_raster_sao0/bin"].tobytes()
    assert len(stream) == 277
    codes = [ok_or_refused(hp, stream[:n]) for n in range(1, len(stream) + 1)]
    # the whole stream is read; a prefix that ends in front of the first byte of slice data holds no picture (behind it the reader cannot tell a cut from the end)
    info, rbsp = hp.access_unit_read_host(stream)[:2]
    vcl_at = [p + len(u) - len(u.lstrip(b"\x00")) + 1 for p, u, t in S.split_units(stream) if t < 32][0]
    assert codes[-1] == 0 and all(c == -1 for c in codes[:vcl_at + info.header_bytes])
    assert codes[vcl_at + info.header_bytes] == 0                          # one byte of slice data: a picture as far as this layer can see


@pytest.mark.parametrize("name,key,stream,method", STREAMS, ids=[s[0] for s in STREAMS])
def test_damaged_streams_are_read_or_refused(name, key, stream, method):
    hp = R.hophip()
    aus = hp.annexb_access_units(stream)
    active = hp.access_unit_read_host(aus[0])[0]
    seen = set()
    for k, au in enumerate(aus):
        for bad in R.damage(au, R.stream_seed(name) + k):
            seen.add(ok_or_refused(hp, bad, active if k else None))
    assert seen <= {0, -1} and len(seen) >= 1


def refused(hp, au, active=None, **kw):
    with pytest.raises(hp.HopError) as e:
        hp.access_unit_read_host(au, active, **kw)
    return e.value.code == -1


def test_refusals():
    hp = R.hophip()
    L = hp.load()
    subs = R.crafted_substreams("drawn", 3)
    nal = R.slice_nal(subs, 1)
    good = R.access_unit(64, 192, nal, 1)
    info = hp.access_unit_read_host(good)[0]
    # NULL arguments
    L.hop_access_unit_read_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_int32, ctypes.c_void_p]
    buf = (ctypes.c_uint8 * 4096)(); n = ctypes.c_size_t(); sz = (ctypes.c_uint32 * 8)(); dg = (ctypes.c_uint8 * 48)(); out = hp.StreamInfo()
    full = [good, len(good), None, ctypes.byref(out), buf, 4096, ctypes.byref(n), sz, 8, dg]
    assert L.hop_access_unit_read_host(*full) == 0
    for k in (0, 3, 4, 6, 7, 9):
        assert L.hop_access_unit_read_host(*[None if i == k else v for i, v in enumerate(full)]) == -1, k
    sets = good[:len(good) - len(nal) - 3]
    assert refused(hp, sets)                                                               # no VCL unit
    assert refused(hp, good + b"\x00\x00\x01" + nal)                                      # more than one
    assert refused(hp, good[:len(sets) + 3 + info.header_bytes - 1])                      # a unit that ends inside an element: the slice header
    assert refused(hp, sets[:-4] + good[len(sets):])                                      # ... the PPS
    assert refused(hp, R.access_unit(64, 192, R.slice_nal(subs, 1, offsets=[200, 500]), 1))   # entry points that sum past the payload
    assert refused(hp, R.access_unit(64, 192, R.slice_nal([b"\x55\x00\x00", b"", b"\x01\x77"], 1, offsets=[3, 1]), 1))   # an empty substream: 55 00 00 | 03 | 01 77
    assert refused(hp, R.access_unit(64, 128, nal, 1))                                    # three substreams in a picture of two CTU rows
    assert refused(hp, R.access_unit(64, 192, R.slice_nal(subs[:1], 1), 1))               # one substream with wpp in a picture of three
    assert refused(hp, good, max_substreams=2)                                            # more substreams than max_substreams
    assert not refused_ok(hp, good, max_substreams=3)
    other = hp.StreamInfo.from_buffer_copy(bytes(info)); other.pic_w = 128
    assert refused(hp, good, other)                                                       # `active` contradicting the parameter sets present
    assert hp.access_unit_read_host(good, info)[1] == b"".join(subs)
    bare = R.access_unit(64, 192, nal, 1, sets=False)
    assert refused(hp, bare)                                                              # `active` missing
    assert hp.access_unit_read_host(bare, info)[1] == b"".join(subs)
    assert refused(hp, R.access_unit(64, 64, R.slice_nal(None, 0, offsets=[], raw_payload=b"\x41\x00\x00\x02\x80"), 0))   # a violation
    assert refused(hp, R.access_unit(64, 64, R.slice_nal(None, 0, offsets=[], raw_payload=b"\x41\x00\x00\x03\x04\x80"), 0))
    assert hp.access_unit_read_host(R.access_unit(64, 64, R.slice_nal(None, 0, offsets=[], raw_payload=b"\x41\x00\x00\x03\x02\x80"), 0))[1] == b"\x41\x00\x00\x02\x80"
    # cabac_zero_words behind the slice data are cut; a constant of the writer with another value is refused; an overflow reports the size
    assert hp.access_unit_read_host(R.access_unit(64, 192, nal + b"\x00\x00\x03\x00\x00\x03", 1))[1] == b"".join(subs)
    assert refused(hp, R.access_unit(64, 192, R.slice_nal(subs, 1, qp=60), 1))
    with pytest.raises(hp.HopError) as e:
        hp.access_unit_read_host(good, capacity=len(b"".join(subs)) - 1)
    assert e.value.code == -1 and e.value.needed == len(b"".join(subs))


def refused_ok(hp, au, **kw):
    try:
        hp.access_unit_read_host(au, **kw)
        return False
    except hp.HopError:
        return True


def test_second_picture_needs_the_first_pictures_info():
    hp = R.hophip()
    aus = hp.annexb_access_units(U.load_fixture()["128x64_2frames/bin"].tobytes())
    assert len(aus) == 2 and refused(hp, aus[1])
    first = hp.access_unit_read_host(aus[0])[0]
    info, rbsp, sizes, digest = hp.access_unit_read_host(aus[1], first)
    assert (info.params.poc, info.params.parameter_sets, info.nal_type) == (1, 0, 0) and len(rbsp) == int(sizes.sum()) > 0
