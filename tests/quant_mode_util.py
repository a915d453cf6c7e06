"""Helpers of the quantiser-mode tests (tests/test_quant_mode_cpu.py, tests/test_gpu_quant_mode.py; hop_ctx_set_quant_mode): the streams of
tests/golden/stream_rdoq0.npz (tools/make_golden_rdoq0.py) -- the unmodified reference encoder's bitstreams of three slice-data cases with --RDOQ=0 --RDOQTS=0, one of
them also with --RDOQ=1 --RDOQTS=0 -- next to the RDOQ-on stream of the same case in tests/golden/slice_data.npz; the blocks of tests/golden/quant_flat.npz and
quant_flat_sbh.npz; and crafted blocks for the corners of TComTrQuant::signBitHidingHDQ.

The crafted blocks are written in SCAN order at a quantiser whose step is a power of two, so that level and remainder can be read off the coefficient:
8 bit, 4x4 at qp_scaled 28 or 8x8 at qp_scaled 34 give qBits = 23 and Q = 2^14: level = (|c| + 85 or 171) >> 9, deltaU = (|c| - 512 * level) >> 1.
4x4 at qp_scaled 4 gives a step of 32 (levels beyond 16 bit from coefficients that fit an Int): level = (|c| + 5 or 10) >> 5, deltaU = (|c| - 32 * level) * 8."""
import ctypes
import os

import numpy as np

import slicedata_util as U
from hoputil import oracle

FIXTURE = os.path.join(U.ROOT, "tests", "golden", "stream_rdoq0.npz")
MODES = {"64x64_raster": ((0, 0),), "136x72_plain10": ((0, 0),), "448x192_seed3_mi15_wpp": ((0, 0), (1, 0))}      # case -> (rdoq, rdoq_ts) of its streams
STREAMS = [(key, m) for key, modes in MODES.items() for m in modes]
IDS = ["%s_rdoq%d%d" % (key, m[0], m[1]) for key, m in STREAMS]
CASES = U.slice_cases()
NLANES = (1, 16, 64, 256, 1024)


def stream(key, mode):
    """the whole .bin (one access unit) of the case coded with (rdoq, rdoq_ts); (1, 1) is slice_data.npz's"""
    if tuple(mode) == (1, 1):
        return U.load_fixture()[key + "/bin"].tobytes()
    return np.load(FIXTURE)["%s_rdoq%d%d/bin" % (key, mode[0], mode[1])].tobytes()


def scan_of(scan_idx, log2):
    O = oracle()
    O.hop_o_scan.restype = ctypes.POINTER(ctypes.c_uint32); O.hop_o_scan.argtypes = [ctypes.c_int, ctypes.c_int]
    p = O.hop_o_scan(scan_idx, log2)
    return np.array([p[i] for i in range(1 << (2 * log2))], np.int64)


def oracle_flat_sbh(coef, bd, qp, is_i, scan_idx, sign_hide=1):
    """hop_o_quant_flat_sbh (or hop_o_quant_flat) of an N x N block: (levels (N, N), abs_sum)"""
    O = oracle()
    O.hop_o_quant_flat_sbh.restype = ctypes.c_uint32; O.hop_o_quant_flat.restype = ctypes.c_uint32
    c = np.ascontiguousarray(coef, np.int32); N = c.shape[0]
    d = np.zeros((N, N), np.int32)
    VP = ctypes.c_void_p
    if sign_hide:
        a = O.hop_o_quant_flat_sbh(int(bd), int(qp), int(is_i), c.ctypes.data_as(VP), d.ctypes.data_as(VP), N, int(scan_idx))
    else:
        a = O.hop_o_quant_flat(int(bd), int(qp), int(is_i), c.ctypes.data_as(VP), d.ctypes.data_as(VP), N)
    return d, int(a)


def in_scan_order(N, scan_idx, values):
    """the N x N block whose coefficient at scan position sp is values[sp] (a dict; the rest zero)"""
    scan = scan_of(scan_idx, N.bit_length() - 1)
    c = np.zeros(N * N, np.int32)
    for sp, v in values.items():
        c[scan[sp]] = v
    return c.reshape(N, N)


def crafted():
    """name -> (N, qp_scaled, {scan position: coefficient}): the corners of signBitHidingHDQ, see the module's docstring for the arithmetic"""
    big = 32 * 40000 + 20
    return {
        # two candidates of equal, least cost (-50) at positions 0 and 5: the descending loop's strict `<` keeps the first it meets, position 5
        "equal_cost": (4, 28, {0: 2 * 512 + 100, 5: 512 + 100}),
        "equal_cost_three": (4, 28, {1: -(3 * 512 + 60), 4: 60, 7: 512 + 60, 9: 2 * 512 + 60}),      # and a zero among them
        # the level 1 at firstNZ would be the cheapest to lower (deltaU -40) and may not be; the next best is the level 2 at position 8 (-5)
        "first_is_one": (4, 28, {2: 512 - 80, 8: 2 * 512 + 10}),
        "first_is_minus_one": (4, 28, {2: -(512 - 80), 8: 2 * 512 + 10, 11: 512 + 2}),
        "only_level_is_one_at_first": (4, 28, {0: 512 + 30}),                                         # one level: nothing to hide in
        # zeros in front of firstNZ: position 0 has the larger remainder and the wrong sign, position 1 the right one
        "zero_in_front_wrong_sign": (4, 28, {0: -300, 1: 200, 3: 3 * 512 + 5, 9: 2 * 512 + 3}),
        "zero_in_front_wrong_sign_neg": (4, 28, {0: 300, 1: -200, 3: -(3 * 512 + 5), 9: 3 * 512 + 4}),
        # levels beyond 16 bit, clipped; the clipped level has the least cost and is changed by -1 whatever its remainder says
        "level_32767": (4, 4, {0: big, 6: 2 * 32 + 1}),
        "level_minus_32768": (4, 4, {0: -big, 6: 2 * 32 + 1}),
        # 8x8, levels in groups 1 and 2, none in group 3: group 2 is the last group and must not look above its last level (position 37 is cheap there),
        # group 1 must (position 30 is cheap there)
        "last_group_and_later": (8, 34, {16: 512 + 10, 22: 2 * 512 + 10, 30: 400, 32: 512 + 10, 36: 2 * 512 + 10, 37: 400}),
        "last_group_is_group_0": (8, 34, {1: 512 + 10, 6: 2 * 512 + 10, 9: 400}),
        "all_zero": (4, 28, {0: 300, 5: -200, 15: 100}),
        "nothing_at_all": (8, 34, {}),
        "abs_sum_one": (4, 28, {7: -(512 + 9)}),
        # first and last level three positions apart (no hiding) in group 0, four apart in group 1
        "spread_3_and_4": (8, 34, {2: 512 + 10, 5: 2 * 512 + 10, 18: 512 + 10, 22: 2 * 512 + 10}),
        "spread_3_only": (4, 28, {4: 512 + 10, 7: 2 * 512 + 10}),
        "spread_4_only": (4, 28, {4: 512 + 10, 8: 2 * 512 + 10}),
    }
