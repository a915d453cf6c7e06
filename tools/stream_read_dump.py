#!/usr/bin/env python3
"""tools/stream_read_dump.py <out.dump> -- the file tools/stream_read_check.cpp reads: records of 8 uint32 and their payload, a record of kind 0 ends the file.

kind 1, an access unit: bytes, seed, has_active, prefixes, then (if has_active) the 64 bytes of the first picture's hop_stream_info, then the bytes.  Every access unit of
the 19 fixture streams (tests/golden/slice_data.npz, stream_hash.npz; seed = stream_read_util.stream_seed(name) + picture, as tests/test_stream_read_cpu.py damages them;
prefixes for 64x64_raster_sao0 only) and the crafted ones of stream_read_util.crafted().
kind 2, an unescape input: n (lookback included), n_seg, lookback, want_len, want_violations, then the segment sizes, the expected per-segment RBSP sizes, the n bytes
and the expected output -- the escaped crafted contents of the tests at every segmentation, and the same contents unescaped as they are, with and without lookback."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stream_read_util as R  # noqa: E402
import stream_util as S  # noqa: E402

hp = R.hophip()
path = sys.argv[1]
n_units = n_une = 0
with open(path, "wb") as f:
    def head(*v):
        f.write(np.array(list(v) + [0] * (8 - len(v)), np.uint32).tobytes())

    for name, key, stream, method in R.streams():
        active = None
        for k, au in enumerate(hp.annexb_access_units(stream)):
            head(1, len(au), R.stream_seed(name) + k, 1 if active is not None else 0, 1 if name == "64x64_raster_sao0" else 0)
            if active is not None:
                f.write(bytes(active))
            f.write(au)
            active = active or hp.access_unit_read_host(au)[0]
            n_units += 1
    for name, au, subs in R.crafted():
        head(1, len(au), R.stream_seed(name), 0, 0); f.write(au); n_units += 1

    def unescape_record(data, back, seg):
        global n_une
        want, sizes, viol = R.position_rule(data, back, seg)
        head(2, len(data), len(seg), back, len(want), viol)
        f.write(np.array(list(seg) + sizes, np.uint32).tobytes()); f.write(data); f.write(want)
        n_une += 1

    for n in S.ESCAPE_LENGTHS:
        for name, a in S.escape_contents(n).items():
            data = a.tobytes()
            esc = S.escape_restated(data)[0]
            esc = esc[:-1] if data[-1] == 0 else esc
            for seg in R.escaped_segmentations(esc):
                unescape_record(esc, 0, seg)
            for back in (0, 1, 2):
                if n > back:
                    unescape_record(data, back, [n - back])
    head(0)
print(n_units, "access units and", n_une, "unescape records ->", path, os.path.getsize(path), "bytes")
