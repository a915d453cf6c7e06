"""CPU: the quantiser of a transform unit that does not use RDOQ (hop_ctx_set_quant_mode; csrc/k_quant_flat_dev.inl) as the host compiles it, and the fixture the device
tests lean on.

hop_quant_flat_tu_host runs the two phases of the leaf step's plain quantiser -- levels and remainders a scan position per lane, sign-bit hiding a coefficient group per
lane -- over emulated lanes.  It must give the levels and the sum of the reference's own xQuant with RDOQ off (tests/golden/quant_flat.npz, quant_flat_sbh.npz: 1000
blocks, every size, 8 / 10 bit, both rounding offsets, the three scans) whatever the number of lanes and their order, and the oracle's restatement of
TComTrQuant::signBitHidingHDQ on blocks crafted for its corners (tests/quant_mode_util.py).

The streams of tests/golden/stream_rdoq0.npz are the unmodified reference encoder's with --RDOQ=0 --RDOQTS=0 (one also with --RDOQ=1 --RDOQTS=0).  The last tests check
the FIXTURE, not the feature: each stream differs from the RDOQ-on stream of its case in the slice alone, and decodes -- reader, parser, the reference decoder of
tests/refdecode.py, the oracle's loop filters -- to the picture whose MD5 its SEI carries.  No device is touched."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import quant_mode_util as Q
import slicedata_util as U
import stream_read_util as R
from goldutil import load
from hoputil import ROOT, oracle, oracle_deblock
from refdecode import ref_decode

LANE_FORMS = [(n, d) for n in Q.NLANES for d in (0, 1)]


def host_all_forms(hp, L, coef, bd, qp, is_i, sign_hide, scan_idx):
    """the yardstick under every lane count and both orders: one (levels, abs_sum), the same bytes from all"""
    first = None
    for nlanes, desc in LANE_FORMS:
        lev, a = hp.quant_flat_tu_host(coef, bd, qp, is_i, sign_hide, scan_idx, nlanes, desc, lib=L)
        if first is None:
            first = (lev, a)
        assert a == first[1] and lev.tobytes() == first[0].tobytes(), (nlanes, desc)
    return first


@pytest.fixture(scope="module")
def lib():
    return R.hophip().load()


def test_golden_blocks_without_sign_hiding(lib):
    hp = R.hophip()
    g = load("quant_flat.npz")
    for N, bd, qp, isI, asum, off in g["par"]:
        N, off = int(N), int(off)
        src = g["src"][off:off + N * N].astype(np.int32).reshape(N, N)
        lev, a = host_all_forms(hp, lib, src, int(bd), int(qp), int(isI), 0, 0)
        assert a == int(asum) and np.array_equal(lev.ravel(), g["out"][off:off + N * N]), (N, bd, qp, isI)


def test_golden_blocks_with_sign_hiding(lib):
    hp = R.hophip()
    g = load("quant_flat_sbh.npz")
    for N, bd, qp, isI, asum, off, scan in g["par"]:
        N, off = int(N), int(off)
        src = g["src"][off:off + N * N].astype(np.int32).reshape(N, N)
        lev, a = host_all_forms(hp, lib, src, int(bd), int(qp), int(isI), 1, int(scan))
        assert a == int(asum) and np.array_equal(lev.ravel(), g["out"][off:off + N * N]), (N, bd, qp, isI, scan)


@pytest.mark.parametrize("name", list(Q.crafted()))
def test_crafted_blocks_equal_the_oracle(lib, name):
    hp = R.hophip()
    N, qp, values = Q.crafted()[name]
    for scan_idx in (0, 1, 2):
        for is_i in (0, 1):
            coef = Q.in_scan_order(N, scan_idx, values)
            want, want_sum = Q.oracle_flat_sbh(coef, 8, qp, is_i, scan_idx)
            lev, a = host_all_forms(hp, lib, coef, 8, qp, is_i, 1, scan_idx)
            assert a == want_sum and np.array_equal(lev, want), (name, scan_idx, is_i, lev.ravel().tolist(), want.ravel().tolist())


def _in_scan(name, scan_idx=0, is_i=0):
    """(levels without hiding, levels with hiding) of a crafted block, both in scan order, from the yardstick"""
    hp = R.hophip()
    N, qp, values = Q.crafted()[name]
    coef = Q.in_scan_order(N, scan_idx, values)
    scan = Q.scan_of(scan_idx, N.bit_length() - 1)
    plain, s0 = hp.quant_flat_tu_host(coef, 8, qp, is_i, 0, scan_idx)
    hidden, s1 = hp.quant_flat_tu_host(coef, 8, qp, is_i, 1, scan_idx)
    assert s0 == s1                                                          # uiAcSum is the sum before the hiding
    return plain.ravel()[scan], hidden.ravel()[scan], s0


def test_crafted_blocks_are_the_corners_they_claim():
    """what each block was crafted for, stated in scan positions (the oracle agrees above; this says that the corner is met at all)"""
    def changed(name, **kw):
        p, h, _ = _in_scan(name, **kw)
        return {int(i): (int(p[i]), int(h[i])) for i in np.nonzero(p != h)[0]}
    assert changed("equal_cost") == {5: (1, 2)}                              # positions 0 and 5 cost the same: the higher one
    assert changed("equal_cost_three") == {9: (2, 3)}
    assert changed("first_is_one") == {8: (2, 3)}                            # not the 1 at firstNZ, although lowering it is cheapest
    assert changed("first_is_minus_one") == {8: (2, 3)}                      # -1 + 2 + 1 is even, the first level negative: hide; again not the -1 (remainder -40)
    assert changed("only_level_is_one_at_first") == {}
    assert changed("zero_in_front_wrong_sign") == {1: (0, 1)}                # position 0 has the larger remainder and the wrong sign
    assert changed("zero_in_front_wrong_sign_neg") == {1: (0, -1)}
    assert changed("level_32767") == {0: (32767, 32766)}
    assert changed("level_minus_32768") == {0: (-32768, -32767)}
    assert _in_scan("level_32767")[2] == 40000 + 2                           # (the sum counts the level before the clip)
    assert changed("last_group_and_later") == {30: (0, 1), 36: (2, 3)}       # group 1 looks above its last level, the last group (2) does not
    assert changed("last_group_is_group_0") == {6: (2, 3)}
    assert changed("all_zero") == {} and _in_scan("all_zero")[2] == 0 and _in_scan("nothing_at_all")[2] == 0
    assert changed("abs_sum_one") == {} and _in_scan("abs_sum_one")[2] == 1
    assert changed("spread_3_and_4") == {22: (2, 3)}
    assert changed("spread_3_only") == {} and changed("spread_4_only") == {8: (2, 3)}


def test_refusals(lib):
    c = np.zeros((4, 4), np.int32); lev = np.zeros((4, 4), np.int32); a = ctypes.c_uint32(0)
    lib.hop_quant_flat_tu_host.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2
    ok = (8, 28, 0, 2, 1, 0)
    assert lib.hop_quant_flat_tu_host(*ok, c.ctypes.data, lev.ctypes.data, ctypes.byref(a), 64, 0) == 0
    for bad in ((7, 28, 0, 2, 1, 0), (8, 88, 0, 2, 1, 0), (8, 28, 0, 1, 1, 0), (8, 28, 0, 6, 1, 0), (8, 28, 0, 2, 1, 3)):
        assert lib.hop_quant_flat_tu_host(*bad, c.ctypes.data, lev.ctypes.data, ctypes.byref(a), 64, 0) == -1, bad
    for nlanes in (0, 1025):
        assert lib.hop_quant_flat_tu_host(*ok, c.ctypes.data, lev.ctypes.data, ctypes.byref(a), nlanes, 0) == -1
    assert lib.hop_quant_flat_tu_host(*ok, None, lev.ctypes.data, ctypes.byref(a), 64, 0) == -1


# ---- the fixture ----
_read = {}


def read(key, mode):
    if (key, mode) not in _read:
        _read[(key, mode)] = R.hophip().access_unit_read_host(Q.stream(key, mode), None)
    return _read[(key, mode)]


def _split(data):
    units = U.nal_units(data)
    kind = [(u[0] >> 1) & 0x3F for u in units]
    return [(k, u) for k, u in zip(kind, units) if k >= 32 and k != 40], [u for k, u in zip(kind, units) if k < 32]


@pytest.mark.parametrize("key", list(Q.MODES))
def test_the_fixture_holds_what_the_tests_lean_on(key):
    """the switch changes the slice and nothing else; every stream of a case is another one"""
    fixed_on, slice_on = _split(Q.stream(key, (1, 1)))
    slices = [slice_on[0]]
    for mode in Q.MODES[key]:
        fixed, sl = _split(Q.stream(key, mode))
        assert fixed == fixed_on and len(sl) == 1, (key, mode)
        slices.append(sl[0])
        s, s_on = read(key, mode)[0].params.slice, read(key, (1, 1))[0].params.slice
        assert [getattr(s, f) for f, _ in s._fields_] == [getattr(s_on, f) for f, _ in s_on._fields_], (key, mode)
    assert len(set(slices)) == len(slices), key


@pytest.mark.parametrize("key,mode", Q.STREAMS, ids=Q.IDS)
def test_fixture_stream_decodes_to_the_picture_its_sei_names(key, mode):
    hp = R.hophip()
    c = Q.CASES[key]
    info, rbsp, sizes, digest = read(key, mode)
    W, H, bd, qp = info.pic_w, info.pic_h, info.bit_depth, info.params.slice.qp
    assert (W, H, bd, info.params.hash) == (c["W"], c["H"], c["bd"], 1)
    parts, levels, sao = hp.slice_data_parse_host(W, H, rbsp, sizes, **R.parse_kwargs(info))
    rec, _ = ref_decode(W, H, parts, levels, qp, 0, 0, bd, 1 if c["plain"] else 0)
    final = [np.ascontiguousarray(a, np.int16) for a in oracle_deblock(W, H, (qp, 0, 0, 0, 0), parts, rec, bd)]
    if sao is not None:
        recon = hp.sao_reconstruct_params(sao, (W + 63) // 64, bd)
        O = oracle()
        P3 = ctypes.c_void_p * 3
        out = [np.zeros_like(a) for a in final]
        O.hop_o_sao_apply.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
        assert O.hop_o_sao_apply(W, H, bd, P3(*[a.ctypes.data for a in final]), recon.ctypes.data_as(ctypes.c_void_p), P3(*[a.ctypes.data for a in out])) == 0
        final = out
    for comp in range(3):
        raw = final[comp].astype(np.uint8).tobytes() if bd == 8 else final[comp].astype("<u2").tobytes()
        assert bytes(digest[comp]) == hashlib.md5(raw).digest(), (key, mode, comp)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tools/quant_flat_check.cpp with host/hop_quant_flat_host.cpp and the scan builder of host/hop_hostlogic.cpp as a program of its own under
    -fsanitize=address,undefined, over the golden and the crafted blocks (tools/quant_flat_dump.py writes them with the expected levels)"""
    import sys
    cases = tmp_path / "blocks.bin"; exe = tmp_path / "quant_flat_check"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "quant_flat_dump.py"), str(cases)])
    H = os.path.join(ROOT, "hevc-hop_amd", "host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "quant_flat_check.cpp"), os.path.join(H, "hop_quant_flat_host.cpp"), os.path.join(H, "hop_hostlogic.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "blocks: 0 wrong" in r.stdout and not r.stdout.startswith("0 blocks"), r.stdout[-2000:]
