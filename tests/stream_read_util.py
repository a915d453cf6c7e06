"""Helpers of the stream-reading tests (tests/test_stream_read_cpu.py, tests/test_gpu_stream_read.py) and of tools/stream_read_dump.py: the fixture streams, the
position rule of the entry points restated, segment cuts around inserted 03s, a Python restatement of the slice header (from the layout in host/hop_stream.cpp) that
wraps crafted substreams into access units, and the seeded damage generator tools/stream_read_check.cpp repeats."""
import importlib.util
import os

import numpy as np

import slicedata_util as U
import stream_util as S

CASES = U.slice_cases()
_hp = None


def hophip():
    global _hp
    if _hp is None:
        spec = importlib.util.spec_from_file_location("hophip", os.path.join(U.ROOT, "hevc-hop_amd", "hophip.py"))
        _hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(_hp)
    return _hp


def streams():
    """[(name, case key, the whole .bin, hash method)]: the 17 MD5 streams of slice_data.npz and the two checksum streams of stream_hash.npz"""
    G, Hs = U.load_fixture(), np.load(S.HASH_FIXTURE)
    return [(k, k, G[k + "/bin"].tobytes(), 1) for k in CASES] + [(k + "_checksum", k, Hs[k + "/bin"].tobytes(), 3) for k in S.HASH_CASES]


def parse_kwargs(info):
    s = info.params.slice
    return dict(bit_depth=info.bit_depth, qp=s.qp, slice_type=s.slice_type, wpp=s.wpp, plain_intra=s.plain_intra, sao_luma=s.sao_luma, sao_chroma=s.sao_chroma, mi_size=s.mi_size)


# ---- the position rule (TDecCAVLC.cpp:1343-1353) restated ----
def position_rule(data, lookback, segments):
    """(the RBSP, per segment its size less the removed bytes whose escaped position lies inside it, violations) of lookback bytes + segments"""
    d = np.concatenate([np.full(2, 255, np.uint8), np.frombuffer(bytes(data), np.uint8), np.zeros(1, np.uint8)])   # (ff in front: no zeros; 00 behind: nothing > 3)
    z2 = (d[:-3] == 0) & (d[1:-2] == 0)                                      # per byte of data: the two bytes in front of it are 00 00
    b, nxt = d[2:-1], d[3:]
    removed = z2 & (b == 3)
    bad = (z2 & (b <= 2)) | (removed & (nxt > 3))
    removed[:lookback] = False; bad[:lookback] = False
    keep = ~removed; keep[:lookback] = False
    edges = lookback + np.concatenate([[0], np.cumsum(np.asarray(segments, np.int64))])
    sizes = [int(hi - lo - removed[lo:hi].sum()) for lo, hi in zip(edges[:-1], edges[1:])]
    return b[keep].tobytes(), sizes, int(bad.sum())


def escaped_segmentations(escaped):
    """the escaped buffer cut at 1, 2 and 7 places; wherever an 03 was inserted (every 00 00 03 of an escaped buffer) the cuts include one directly in front of it and
    one directly behind it (the nearest to the even cut)"""
    n = len(escaped)
    a = np.frombuffer(escaped, np.uint8)
    ins = np.flatnonzero((a[2:] == 3) & (a[1:-1] == 0) & (a[:-2] == 0)) + 2 if n > 2 else np.zeros(0, np.int64)
    out = []
    for places in (1, 2, 7):
        if n <= places:
            continue
        for side in (0, 1):
            cuts = set()
            for k in range(1, places + 1):
                want = k * n // (places + 1)
                if len(ins):
                    want = int(ins[np.argmin(np.abs(ins - want))]) + side
                cuts.add(min(max(want, 1), n - 1))
            edges = [0] + sorted(cuts) + [n]
            seg = [b - a_ for a_, b in zip(edges[:-1], edges[1:])]
            if seg not in out:
                out.append(seg)
    return out or [[n]]


# ---- the slice header restated: a bit writer and the layout of hop_strm_slice_header ----
class Bits:
    def __init__(self):
        self.bits = []

    def code(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n - 1, -1, -1)]

    def ue(self, v):
        n = (v + 1).bit_length() - 1
        self.code(0, n); self.code(v + 1, n + 1)

    def se(self, v):
        self.ue(-2 * v if v <= 0 else 2 * v - 1)

    def trailing(self):
        self.code(1, 1)
        while len(self.bits) % 8:
            self.code(0, 1)

    def bytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(int("".join(map(str, self.bits[i:i + 8])), 2) for i in range(0, len(self.bits), 8))


def slice_header(wpp, offsets, len_m1=None, qp=32, plain=0, sao=(1, 1), poc=0):
    """the NAL unit header and the slice segment header up to its byte alignment, as RBSP; offsets: the entry points (escaped bytes), len_m1: offset_len_minus1
    (default: what the largest offset takes)"""
    w = Bits()
    w.code(0, 1); w.code(19 if poc == 0 else (1 if plain else 0), 6); w.code(0, 6); w.code(1, 3)
    w.code(1, 1)
    if poc == 0:
        w.code(0, 1)
    w.ue(0); w.ue(2)
    if poc:
        w.code(poc & 255, 8); w.code(1, 1); w.code(0, 1); w.code(1 if plain else 0, 1)
    if sao[0] or sao[1]:
        w.code(sao[0], 1); w.code(sao[1], 1)
    if not plain:
        w.code(1, 1); w.ue(0); w.ue(0)
    w.se(qp - 26)
    w.code(1, 1)
    if wpp:
        w.ue(len(offsets))
        if offsets:
            if len_m1 is None:
                len_m1 = max(max(offsets).bit_length(), 1) - 1
            w.ue(len_m1)
            for o in offsets:
                w.code(o - 1, len_m1 + 1)
    w.trailing()
    return w.bytes()


def slice_nal(subs, wpp, offsets=None, raw_payload=None, **header):
    """the escaped VCL NAL unit around substreams that each end in a non-zero byte; offsets: default the escaped length of each substream but the last; raw_payload: bytes
    put behind the escaped header as they are instead of the escaped substreams"""
    if offsets is None:
        offsets = [len(S.escape_restated(s)[0]) for s in subs[:-1]]
    head = slice_header(wpp, offsets, **header)
    if raw_payload is not None:
        return S.escape_restated(head)[0] + raw_payload
    return S.escape_restated(head + b"".join(subs))[0]


def access_unit(W, H, nal, wpp, plain=0, sao=1, mi=16, bd=8, sets=True):
    hp = hophip()
    ps = hp.parameter_sets_write(W, H, bit_depth=bd, slice_type=2 if plain else 3, wpp=wpp, plain_intra=plain, sao=sao, mi_size=mi) if sets else b"\x00"
    return ps + b"\x00\x00\x01" + nal


def crafted_substreams(kind, n_sub, n=600):
    """n bytes of stream_util.escape_contents' `kind` cut into n_sub substreams, each made to end in a non-zero byte"""
    a = S.escape_contents(n)[kind].copy()
    edges = [k * n // n_sub for k in range(n_sub + 1)]
    subs = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        s = a[lo:hi].copy()
        if s[-1] == 0:
            s[-1] = 0x80
        subs.append(s.tobytes())
    return subs


def crafted_access_units():
    """[(name, access unit, the substreams it must read back as)]: 1 / 3 / 6 substreams of "drawn" and "runs" bytes in pictures of as many CTU rows; six one-byte
    substreams behind 16-bit entry points of 1, whose zero words force 03s INTO the slice header; a substream ending in 00 00 in front of one starting with 01, the
    boundary in front of and behind the inserted 03"""
    out = []
    for kind in ("drawn", "runs"):
        for n_sub in (1, 3, 6):
            subs = crafted_substreams(kind, n_sub)
            wpp = 1 if n_sub > 1 else 0
            out.append(("%s_%d" % (kind, n_sub), access_unit(64, 64 * n_sub, slice_nal(subs, wpp), wpp), subs))
    subs = [bytes([0x81 + k]) for k in range(6)]
    nal = slice_nal(subs, 1, len_m1=15)
    assert b"\x00\x00\x03" in nal[:-6]
    out.append(("header_03", access_unit(64, 384, nal, 1), subs))
    subs = [b"\x55\x66\x00\x00", b"\x01\x77\x88", b"\x99"]
    for name, first in (("boundary_front", 4), ("boundary_behind", 5)):       # 55 66 00 00 | 03 | 01 77 88 | 99: the 03 opens the second segment, or closes the first
        out.append((name, access_unit(64, 192, slice_nal(subs, 1, offsets=[first, 8 - first]), 1), subs))
    return out


_crafted = None


def crafted():
    global _crafted
    if _crafted is None:
        _crafted = crafted_access_units()
    return _crafted


# ---- damage: the generator tools/stream_read_check.cpp repeats ----
def damage(au, seed, count=100):
    """count copies of au with one byte changed each: x <- 1664525 x + 1013904223 (mod 2^32) from x = seed; position (x >> 8) % len, then the next x gives the value
    (x >> 16) & 255, its lowest bit flipped when that is the byte already there"""
    x = seed & 0xffffffff
    for _ in range(count):
        x = (1664525 * x + 1013904223) & 0xffffffff
        pos = (x >> 8) % len(au)
        x = (1664525 * x + 1013904223) & 0xffffffff
        v = (x >> 16) & 255
        if v == au[pos]:
            v ^= 1
        yield au[:pos] + bytes([v]) + au[pos + 1:]


def stream_seed(name):
    """a seed per stream that both languages compute: the sum of the name's bytes"""
    return sum(name.encode())
