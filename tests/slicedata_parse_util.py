"""Helpers of the slice-data parser's tests (tests/test_slicedata_parse_cpu.py, tests/test_gpu_slicedata_parse.py): the comparison of parsed parts with the encoder's
and its one mask rule, and the deterministic damaged streams that tools/slicedata_parse_check.cpp runs under the sanitizers as well (same generator, same seeds)."""
import importlib.util
import os

import numpy as np

from hoputil import ROOT

_hp = None


def hophip():
    global _hp
    if _hp is None:
        spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
        _hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(_hp)
    return _hp


def parse_kwargs(c, **over):
    """the keyword arguments of slice_data_parse / slice_data_parse_host for a case of slicedata_util.slice_cases()"""
    kw = dict(qp=c["qp"], slice_type=c["slice_type"], wpp=c["wpp"], plain_intra=1 if c["plain"] else 0, sao_luma=c["sao"], sao_chroma=c["sao"], mi_size=c["mi"])
    kw.update(over)
    return kw


def _zidx(x4, y4):
    z = 0
    for b in range(4):
        z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1))
    return z


_ZPOS = {_zidx(x, y): (x, y) for x in range(16) for y in range(16)}


def pu_first_units(ctu):
    """the units of one CTU (256 CU_PART records) that are the first unit of a PU of an SS / GT CU"""
    first = np.zeros(256, bool)
    z = 0
    while z < 256:
        u = ctu[z]
        if u["pred_mode"] == 15:
            z += 1
            continue
        n = 256 >> (2 * int(u["depth"]))
        if u["pred_mode"] == 0:
            first[z] = True
            s4, e = (64 >> int(u["depth"])) >> 2, int(u["part_size"])        # the CU's size in units; TComDataCU::getPartIndexAndSize for the second PU
            off = {1: (0, s4 >> 1), 2: (s4 >> 1, 0), 4: (0, s4 >> 2), 5: (0, (s4 >> 2) + (s4 >> 1)), 6: (s4 >> 2, 0), 7: ((s4 >> 2) + (s4 >> 1), 0)}.get(e)
            if off:
                x4, y4 = _ZPOS[z]
                first[_zidx(x4 + off[0], y4 + off[1])] = True
        z += n
    return first


def masked(got, want):
    """`got` with the one field the stream does not carry on every unit taken from `want`: gt_flag on the units of an SS / GT CU that are not a PU's first unit.
    The stream carries one flag per PU, the writer reads the first unit's, the parser stores the PU's flag on all its units; the encoder's parts may hold 0 on another
    unit of a PU with GT (the reference's encoder clears the flag of the unit with the PU's NUMBER, include/hophip.h).  Everything else -- all 40 bytes of every unit,
    used or not -- is compared as it is."""
    out = got.copy()
    for a in range(want.shape[0]):
        keep = pu_first_units(want[a])
        inter = (want[a]["pred_mode"] == 0)
        free = inter & ~keep
        out[a]["gt_flag"][free] = want[a]["gt_flag"][free]
    return out


def assert_parts_equal(got, want, what):
    m = masked(got, want)
    if m.tobytes() == want.tobytes():
        return
    for f in want.dtype.names:
        bad = np.argwhere((m[f] != want[f]).reshape(want.shape[0], 256, -1).any(axis=2))
        if len(bad):
            a, z = (int(v) for v in bad[0])
            raise AssertionError("%s: %s differs on %d units, first CTU %d unit %d: parsed %s, expected %s" % (what, f, len(bad), a, z, m[a, z][f], want[a, z][f]))
    raise AssertionError(what + ": padding differs")


# ---- damaged streams: the generator tools/slicedata_parse_check.cpp restates ----
class Lcg:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.s >> 33


def case_seed(W, H):
    return W * 65536 + H


def variants(data, sizes, seed, count=100):
    """count damaged forms of (data, sizes): variant i is of kind i % 5 -- 0 one byte replaced, 1 one bit flipped, 2 a tail of zeros, 3 a tail of 0xFF, 4 the sizes of two
    substreams exchanged (a picture of one substream: a bit flip instead).  Two draws per variant, whatever the kind."""
    g = Lcg(seed)
    n, ns = len(data), len(sizes)
    for i in range(count):
        r1, r2 = g.next(), g.next()
        d = bytearray(data); s = np.array(sizes, np.uint32)
        kind = i % 5
        if kind == 4 and ns < 2:
            kind = 1
        if kind == 0:
            d[r1 % n] = r2 & 255
        elif kind == 1:
            d[r1 % n] ^= 1 << (r2 % 8)
        elif kind == 2:
            d[r1 % n:] = bytes(n - r1 % n)
        elif kind == 3:
            d[r1 % n:] = b"\xff" * (n - r1 % n)
        else:
            a = r1 % ns; b = (a + 1 + r2 % (ns - 1)) % ns
            s[a], s[b] = s[b], s[a]
        yield i, kind, bytes(d), s
