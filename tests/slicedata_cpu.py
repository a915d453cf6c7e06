"""The CPU path to a picture's slice data, for tests/test_slicedata_cpu.py and tools/make_golden_slicedata.py: the RD spine over the CPU restatement
(oracle/libhop_spine_cpu.so) gives the partition data and the levels, the restated loop filter and SAO statistics with the product's SAO decision (hop_sao_decide) give the
coded SAO parameters -- the path oracle/enc_shim_pic.cpp takes --, and hop_slice_data_write_host writes the bytes."""
import ctypes
import os

import numpy as np

from hoputil import ROOT, SAO_PARAM_DTYPE, SaoParams, oracle, oracle_deblock
from slicedata_util import params_of, sao_lambdas
from test_spine_cpu import PART_DT, cpu_last_levels, cpu_last_rd_fraction, run_cpu, run_cpu_plain, run_cpu_wpp, spine_cpu

_lib = None


def hophip_host():
    """libhophip.so for its host-only entries (no device is touched)"""
    global _lib
    if _lib is None:
        L = ctypes.CDLL(os.path.join(ROOT, "hevc-hop_amd", "libhophip.so"))
        L.hop_slice_data_write_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        L.hop_sao_decide.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
        _lib = L
    return _lib


def cpu_affordable(c):
    """the pictures the CPU spine codes in some seconds"""
    return c["W"] * c["H"] <= 200 * 136


_coded = {}


def cpu_picture(c, picture=0):
    """parts (n_ctu, 256) PART_DT, levels (n_ctu, 6144) int32, coded SAO parameters (n_ctu, 3) or None; cached per case and picture"""
    key = (c["W"], c["H"], c["qp"], c["bd"], c["mi"], c["wpp"], c["sao"], picture, c["pictures"][picture][0].tobytes())
    if key in _coded:
        return _coded[key]
    L = spine_cpu()
    W, H = c["W"], c["H"]
    Y, Cb, Cr = c["pictures"][picture]
    n = ((W + 63) // 64) * ((H + 63) // 64)
    if c["plain"]:
        _, _, _, parts, rec, _ = run_cpu_plain(L, W, H, Y, Cb, Cr, c["qp"], c["bd"])
    elif c["wpp"]:
        _, _, _, parts, rec, _, _ = run_cpu_wpp(L, W, H, Y, Cb, Cr, 5, c["qp"], c["mi"])     # the rows as a wavefront, as the picture-level binding runs them
    else:
        _, _, _, parts, rec, _ = run_cpu(L, W, H, Y, Cb, Cr, c["qp"], c["mi"])
    levels = cpu_last_levels(L, n)
    frac = cpu_last_rd_fraction(L, n)
    sao = None
    if c["sao"]:
        O = oracle()
        dbk = oracle_deblock(W, H, (c["qp"], 0, 0, 0, 0), parts, rec, c["bd"])
        org = [np.ascontiguousarray(p, np.int16) for p in (Y, Cb, Cr)]
        stats = np.zeros((n, 3, 5, 32, 2), np.int32)
        P3 = ctypes.c_void_p * 3
        O.hop_o_sao_stats.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
        assert O.hop_o_sao_stats(W, H, c["bd"], P3(*[a.ctypes.data for a in dbk]), P3(*[a.ctypes.data for a in org]), stats.ctypes.data) == 0
        sp = SaoParams((ctypes.c_double * 3)(*sao_lambdas(c["qp"])), (ctypes.c_int32 * 3)(1, 1, 1), c["slice_type"], c["qp"], int(frac[-1]))
        sao = np.zeros((n, 3), SAO_PARAM_DTYPE); recon = np.zeros((n, 3), SAO_PARAM_DTYPE)
        assert hophip_host().hop_sao_decide(n, (W + 63) // 64, c["bd"], stats.ctypes.data, ctypes.byref(sp), sao.ctypes.data, recon.ctypes.data) == 0
    _coded[key] = (parts, levels, sao)
    return _coded[key]


def write_host(c, parts, levels, sao, capacity=1 << 20, guard=0, params=None):
    """hop_slice_data_write_host: (status, bytes written into a buffer of `capacity`, the buffer's `guard` bytes behind it, substream sizes, n_substreams as returned)"""
    L = hophip_host()
    buf = np.full(capacity + guard, 0xA5, np.uint8)
    rows = (c["H"] + 63) // 64
    sizes = np.zeros(rows, np.uint32)
    nsub = ctypes.c_int32(-1)
    p = params or params_of(c)
    rc = L.hop_slice_data_write_host(c["W"], c["H"], c["bd"], ctypes.byref(p), parts.ctypes.data, None if levels is None else levels.ctypes.data,
                                     None if sao is None else sao.ctypes.data, buf.ctypes.data, capacity, sizes.ctypes.data, ctypes.byref(nsub))
    return rc, buf[:capacity], buf[capacity:], sizes, nsub.value


def host_slice_data(c, picture=0):
    """the slice data of one picture of the case through the CPU path: (bytes, substream sizes)"""
    parts, levels, sao = cpu_picture(c, picture)
    rc, buf, _, sizes, nsub = write_host(c, parts, levels, sao)
    assert rc == 0 and nsub == c["rows"], (rc, nsub)
    total = int(sizes[:nsub].sum())
    return buf[:total].tobytes(), sizes[:nsub].copy()
