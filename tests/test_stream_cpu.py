"""CPU: the outer layer of the stream (host/hop_stream.cpp) -- parameter sets, slice header with entry points, decoded-picture-hash SEI, NAL framing, emulation
prevention -- byte for byte against the WHOLE bitstreams of the unmodified reference encoder (tests/golden/slice_data.npz "<key>/bin"; tests/golden/stream_hash.npz for the
checksum hash, tools/make_golden_stream.py).

The pictures come from the CPU path (stream_util.cpu_final_picture: the RD spine over the CPU restatement, the oracle's loop filters with the product's SAO decision), so
the MD5 digests inside the expected SEI also hold the final reconstruction to the reference's.  No device is touched."""
import numpy as np
import pytest

import slicedata_util as U
import stream_util as S
from slicedata_cpu import cpu_affordable

CASES = U.slice_cases()
AFFORDABLE = [k for k, c in CASES.items() if cpu_affordable(c)]


@pytest.fixture(scope="module")
def fixture():
    return U.load_fixture()


@pytest.mark.parametrize("key", list(CASES))
def test_parameter_sets_equal_the_reference_stream(fixture, key):
    c = CASES[key]
    units = S.split_units(fixture[key + "/bin"].tobytes())
    assert [t for _, _, t in units[:3]] == [32, 33, 34]
    want = b"".join(u for _, u, _ in units[:3])
    rc, got, n = S.parameter_sets(c)
    assert rc == 0 and n == len(got)
    assert got == want, S.first_difference(got, want)


def test_the_parameter_sets_hold_emulation_prevention_bytes(fixture):
    """(so the test above pins the host escape as well)"""
    units = S.split_units(fixture["64x64_raster/bin"].tobytes())
    assert b"\x00\x00\x03" in units[0][1][4:] and b"\x00\x00\x03" in units[1][1][4:]


def whole_stream(c, hash):
    out = b""
    for k in range(c["frames"]):
        parts, levels, sao, rec = S.cpu_final_picture(c, k)
        rc, au, n, _ = S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, k, hash))
        assert rc == 0 and n == len(au), (rc, n)
        out += au
    return out


@pytest.mark.parametrize("key", AFFORDABLE)
def test_whole_stream_equals_the_reference_encoder(fixture, key):
    want = fixture[key + "/bin"].tobytes()
    got = whole_stream(CASES[key], 1)
    assert got == want, "%s: %s" % (key, S.first_difference(got, want))


@pytest.mark.parametrize("key", S.HASH_CASES)
def test_checksum_stream_equals_the_reference_encoder(key):
    want = np.load(S.HASH_FIXTURE)[key + "/bin"].tobytes()
    got = whole_stream(CASES[key], 3)
    assert got == want, "%s: %s" % (key, S.first_difference(got, want))


def test_restated_escape_is_the_inverse_of_the_strip():
    for n in (1, 2, 3, 4, 17, 257, 4097):
        for name, a in S.escape_contents(n).items():
            e, cnt = S.escape_restated(a.tobytes())
            stripped = U.strip_emulation_prevention(e)
            # (the final 03 behind a trailing 00 is no emulation prevention byte to the strip unless two zeros precede it: it may stay)
            assert stripped == a.tobytes() or (a[-1] == 0 and e[-1] == 3 and stripped == a.tobytes() + b"\x03"), (n, name)
            assert len(e) == n + cnt + (1 if a[-1] == 0 else 0)
            body = e[:-1] if a[-1] == 0 else e
            assert all(body[i:i + 3] not in (b"\x00\x00\x00", b"\x00\x00\x01", b"\x00\x00\x02") for i in range(len(body) - 2)), (n, name)


@pytest.mark.parametrize("n", S.ESCAPE_LENGTHS)
def test_host_escape_equals_the_restatement(n):
    for name, a in S.escape_contents(n).items():
        data = a.tobytes()
        want, _ = S.escape_restated(data)
        for seg in S.escape_segmentations(a, n):
            rc, got, m, cnt, _ = S.escape_host(data, seg)
            assert rc == 0 and m == len(want) and got == want, (n, name, seg)
            at = 0
            for k, s in enumerate(seg):                                     # per segment: the count of the segment ALONE
                assert cnt[k] == S.escape_restated(data[at:at + s])[1], (n, name, seg, k)
                at += s
    # one byte short: nothing behind the capacity is touched, the size needed is reported
    data = S.escape_contents(n)["zeros"].tobytes()
    want, _ = S.escape_restated(data)
    rc, got, m, _, guard = S.escape_host(data, [n], capacity=len(want) - 1, guard=64)
    assert rc == -1 and m == len(want) and np.all(guard == 0xA5) and got == want[:-1]


def test_escape_refuses_empty_segments():
    assert S.escape_host(b"\x01\x02", [2, 0])[0] == -1
    assert S.escape_host(b"", [])[0] == -1
    assert S.escape_host(b"", [0])[0] == -1


def test_refusals():
    c = CASES["64x64_raster"]
    parts, levels, sao, rec = S.cpu_final_picture(c, 0)
    ok = S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 1))
    assert ok[0] == 0
    assert S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 2))[0] == -1          # CRC
    assert S.access_unit_host(c, parts, levels, sao, None, S.stream_params(c, 0, 1))[0] == -1         # a hash without the reconstruction
    assert S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 0))[0] == -1          # and the reconstruction without a hash
    none = S.access_unit_host(c, parts, levels, sao, None, S.stream_params(c, 0, 0))
    assert none[0] == 0 and ok[1].startswith(none[1]) and S.split_units(ok[1])[-1][2] == 40 and len(S.split_units(none[1])) == 4
    rc, got, n, guard = S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 1), capacity=len(ok[1]) - 1, guard=64)
    assert rc == -1 and n == len(ok[1]) and np.all(guard == 0xA5)                                     # one byte short
    rc, got, n, guard = S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 1), capacity=len(ok[1]), guard=64)
    assert rc == 0 and got == ok[1] and np.all(guard == 0xA5)
    assert S.access_unit_host(c, parts, levels, sao, rec, S.stream_params(c, 0, 1), W=100)[0] == -1   # a width of 100
    assert S.parameter_sets(c, W=100)[0] == -1
    assert S.parameter_sets(c, bd=9)[0] == -1
    rc, got, n = S.parameter_sets(c, capacity=10)
    assert rc == -1 and n == len(S.parameter_sets(c)[1])
