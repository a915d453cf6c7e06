"""Helpers of the stream tests (tests/test_stream_cpu.py, tests/test_gpu_stream.py) and of tools/make_golden_stream.py: the ctypes view of hop_stream_params, the host
entries of the outer layer, the cut of an Annex B stream into its NAL units WITH their start codes, the sequential restatement of emulation prevention, the crafted escape
inputs, and the CPU path to a picture's final reconstruction.

The expected bytes are the whole .bin files of the unmodified reference encoder: tests/golden/slice_data.npz ("<key>/bin", decoded picture hash MD5) and
tests/golden/stream_hash.npz (two of the cases with the checksum hash)."""
import ctypes
import os

import numpy as np

import slicedata_util as U
from hoputil import ROOT, SAO_PARAM_DTYPE, oracle, oracle_deblock

HASH_FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_hash.npz")
HASH_CASES = ("64x64_raster", "136x72_plain10")


class StreamParams(ctypes.Structure):                                        # hop_stream_params
    _fields_ = [("slice", U.SliceDataParams), ("poc", ctypes.c_int32), ("parameter_sets", ctypes.c_int32), ("hash", ctypes.c_int32)]


def stream_params(c, picture=0, hash=1):
    """the reference codes picture 0 as the IDR picture behind the parameter sets, every later one without them"""
    return StreamParams(U.params_of(c), picture, 1 if picture == 0 else 0, hash)


_lib = None


def host_lib():
    """libhophip.so for its host-only entries (no device is touched)"""
    global _lib
    if _lib is None:
        L = ctypes.CDLL(os.path.join(ROOT, "hevc-hop_amd", "libhophip.so"))
        L.hop_parameter_sets_write.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
        L.hop_access_unit_write_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
        L.hop_rbsp_escape_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.hop_sao_decide.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
        _lib = L
    return _lib


def parameter_sets(c, W=None, H=None, bd=None, params=None, capacity=256):
    """hop_parameter_sets_write: (status, bytes, length reported)"""
    p = params or stream_params(c)
    buf = np.full(capacity + 16, 0xA5, np.uint8); n = ctypes.c_size_t(0)
    rc = host_lib().hop_parameter_sets_write(W or c["W"], H or c["H"], bd or c["bd"], ctypes.byref(p), buf.ctypes.data, capacity, ctypes.byref(n))
    assert np.all(buf[capacity:] == 0xA5)
    return rc, buf[:min(n.value, capacity)].tobytes(), n.value


def access_unit_host(c, parts, levels, sao, rec, params, capacity=1 << 20, guard=0, W=None):
    """hop_access_unit_write_host: (status, the bytes, the length reported, the guard bytes behind the buffer)"""
    buf = np.full(capacity + guard, 0xA5, np.uint8); n = ctypes.c_size_t(0)
    planes = None
    if rec is not None:
        keep = [np.ascontiguousarray(a, np.int16) for a in rec]
        planes = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in keep])
    rc = host_lib().hop_access_unit_write_host(W or c["W"], c["H"], c["bd"], ctypes.byref(params), parts.ctypes.data, levels.ctypes.data, None if sao is None else sao.ctypes.data,
                                               planes, buf.ctypes.data, capacity, ctypes.byref(n))
    return rc, buf[:min(n.value, capacity)].tobytes(), n.value, buf[capacity:]


# ---- the stream: NAL units with their start codes ----
def split_units(data):
    """[(offset, bytes including the start code with its zero_byte, nal_unit_type)] of an Annex B stream"""
    data = bytes(data)
    pos = []
    i = data.find(b"\x00\x00\x01")
    while i >= 0:
        pos.append(i - 1 if i > 0 and data[i - 1] == 0 else i)
        i = data.find(b"\x00\x00\x01", i + 3)
    out = []
    for k, p in enumerate(pos):
        end = pos[k + 1] if k + 1 < len(pos) else len(data)
        u = data[p:end]
        out.append((p, u, (u[u.find(b"\x00\x00\x01") + 3] >> 1) & 0x3F))
    return out


def first_difference(got, want):
    """a description of the first differing byte and the NAL unit of the expected stream it lies in; None when equal"""
    if got == want:
        return None
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    unit = [(k, t, p) for k, (p, u, t) in enumerate(split_units(want)) if p <= at]
    k, t, p = unit[-1] if unit else (-1, -1, 0)
    return "first difference at byte %d of %d (got %d bytes): NAL unit %d (type %d), byte %d of it; got %s want %s" % (
        at, len(want), len(got), k, t, at - p, got[at:at + 8].hex(), want[at:at + 8].hex())


# ---- emulation prevention restated: the plain sequential rule ----
def escape_restated(data):
    """a zero counter; 03 in front of a byte <= 3 when the counter is 2; a final 03 after a trailing 00.  Returns (bytes, insertions without the final one)"""
    out, zeros, cnt = bytearray(), 0, 0
    for b in data:
        if zeros == 2 and b <= 3:
            out.append(3); zeros = 0; cnt += 1
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    if len(data) and data[-1] == 0:
        out.append(3)
    return bytes(out), cnt


def escape_host(data, segments, capacity=None, guard=0, want_counts=True):
    """hop_rbsp_escape_host: (status, bytes, length reported, per-segment counts, guard bytes)"""
    a = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    seg = np.asarray(segments, np.uint32)
    cap = len(data) * 3 // 2 + 2 if capacity is None else capacity
    buf = np.full(cap + guard, 0xA5, np.uint8); n = ctypes.c_size_t(0); cnt = np.zeros(max(1, len(seg)), np.uint32)
    rc = host_lib().hop_rbsp_escape_host(a.ctypes.data, seg.ctypes.data, len(seg), buf.ctypes.data, cap, ctypes.byref(n), cnt.ctypes.data if want_counts else None)
    return rc, buf[:min(n.value, cap)].tobytes(), n.value, cnt[:len(seg)], buf[cap:]


ESCAPE_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 70000)


def escape_contents(n):
    """name -> n bytes: the crafted inputs of the escape tests"""
    rng = np.random.RandomState(1000 + n % 997)
    out = {"zeros": np.zeros(n, np.uint8), "001": np.tile(np.array([0, 0, 1], np.uint8), n // 3 + 1)[:n],
           "drawn": np.array([0, 0, 0, 1, 2, 3, 4, 255], np.uint8)[rng.randint(0, 8, n)]}
    runs = []
    for length in range(1, 41):
        for t in (1, 3, 4):
            runs += [0] * length + [t]
    out["runs"] = np.tile(np.array(runs, np.uint8), n // len(runs) + 1)[:n]
    for name, length in (("straddle_even", 4), ("straddle_odd", 5)):          # nothing to escape but one run across every power-of-two offset from 16 to 4096
        st = rng.randint(5, 256, n).astype(np.uint8)
        for k in range(4, 13):
            p = 1 << k
            if p - 2 + length < n:
                st[p - 2:p - 2 + length] = 0; st[p - 2 + length] = 1 + k % 3
        out[name] = st
    for name, tail in (("tail0", [0]), ("tail00", [0, 0]), ("tail003", [0, 0, 3]), ("tail004", [0, 0, 4])):
        a = rng.randint(1, 256, n).astype(np.uint8)
        if n >= len(tail):
            a[n - len(tail):] = tail
        out[name] = a
    return out


def escape_segmentations(data, n):
    """the buffer cut into 1, 2 and 7 segments (fewer where it is shorter), cuts inside zero runs where there are any"""
    out = [[n]]
    zeros = np.flatnonzero((np.asarray(data[:-1]) == 0) & (np.asarray(data[1:]) == 0)) + 1 if n > 1 else []
    for parts in (2, 7):
        if n < parts:
            continue
        cuts = set()
        for k in range(1, parts):
            want = k * n // parts
            if len(zeros):
                want = int(zeros[np.argmin(np.abs(zeros - want))])
            cuts.add(min(max(want, 1), n - 1))
        edges = [0] + sorted(cuts) + [n]
        out.append([b - a for a, b in zip(edges[:-1], edges[1:])])
    return out


# ---- the CPU path to parts, levels, SAO parameters and the FINAL reconstruction of a picture (what tests/test_oracle_golden7.py drives: the oracle's deblocking, its
# SAO statistics, the product's decision hop_sao_decide, the oracle's offsetting pass) ----
_final = {}


def cpu_final_picture(c, picture=0):
    """(parts, levels, coded SAO parameters or None, [Y, Cb, Cr] final reconstruction); cached"""
    key = (c["W"], c["H"], c["qp"], c["bd"], c["mi"], c["wpp"], c["sao"], c["pictures"][picture][0].tobytes())
    if key in _final:
        return _final[key]
    from hoputil import SaoParams
    from test_spine_cpu import cpu_last_levels, cpu_last_rd_fraction, run_cpu, run_cpu_plain, run_cpu_wpp, spine_cpu
    L = spine_cpu()
    W, H = c["W"], c["H"]
    Y, Cb, Cr = c["pictures"][picture]
    n = ((W + 63) // 64) * ((H + 63) // 64)
    if c["plain"]:
        parts, rec = run_cpu_plain(L, W, H, Y, Cb, Cr, c["qp"], c["bd"])[3:5]
    elif c["wpp"]:
        parts, rec = run_cpu_wpp(L, W, H, Y, Cb, Cr, 5, c["qp"], c["mi"])[3:5]
    else:
        parts, rec = run_cpu(L, W, H, Y, Cb, Cr, c["qp"], c["mi"])[3:5]
    levels = cpu_last_levels(L, n); frac = cpu_last_rd_fraction(L, n)
    final = oracle_deblock(W, H, (c["qp"], 0, 0, 0, 0), parts, rec, c["bd"])
    sao = None
    if c["sao"]:
        O = oracle()
        P3 = ctypes.c_void_p * 3
        org = [np.ascontiguousarray(p, np.int16) for p in (Y, Cb, Cr)]
        stats = np.zeros((n, 3, 5, 32, 2), np.int32)
        O.hop_o_sao_stats.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
        assert O.hop_o_sao_stats(W, H, c["bd"], P3(*[a.ctypes.data for a in final]), P3(*[a.ctypes.data for a in org]), stats.ctypes.data) == 0
        sp = SaoParams((ctypes.c_double * 3)(*U.sao_lambdas(c["qp"])), (ctypes.c_int32 * 3)(1, 1, 1), c["slice_type"], c["qp"], int(frac[-1]))
        sao = np.zeros((n, 3), SAO_PARAM_DTYPE); recon = np.zeros((n, 3), SAO_PARAM_DTYPE)
        assert host_lib().hop_sao_decide(n, (W + 63) // 64, c["bd"], stats.ctypes.data, ctypes.byref(sp), sao.ctypes.data, recon.ctypes.data) == 0
        out = [np.zeros_like(a) for a in final]
        O.hop_o_sao_apply.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
        assert O.hop_o_sao_apply(W, H, c["bd"], P3(*[a.ctypes.data for a in final]), recon.ctypes.data_as(ctypes.c_void_p), P3(*[a.ctypes.data for a in out])) == 0
        final = out
    _final[key] = (parts, levels, sao, final)
    return _final[key]
