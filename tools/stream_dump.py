#!/usr/bin/env python3
"""tools/stream_dump.py <case> <picture> <out.dump> | --escape <out.dump> -- the files tools/stream_host_check.cpp reads.

<case> <picture>: one picture of a fixture case of tests/slicedata_util.py coded on the CPU (tests/stream_util.cpu_final_picture) with, as the expected bytes, that
picture's access unit in the reference encoder's own stream (tests/golden/slice_data.npz).  The file: 16 int32 -- pic_w, pic_h, bit_depth, the 7 fields of
hop_slice_data_params, poc, parameter_sets, hash, n_ctu, has_sao, n_bytes --, 256 hop_cu_part per CTU, 6144 int32 levels per CTU, 3 hop_sao_param per CTU if has_sao, the
final reconstruction planes (int16), n_bytes of expected access unit.

--escape: the crafted escape inputs of the tests (stream_util.escape_contents / escape_segmentations) with the sequential restatement's results.  Per record: n, n_seg,
want_len (uint32), the segment sizes and the per-segment counts (uint32 each), n bytes of input, want_len bytes of output; a record with n = 0 ends the file.

Build container only (the CPU spine library)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402
import stream_util as S  # noqa: E402

if sys.argv[1] == "--escape":
    path = sys.argv[2]
    n_rec = 0
    with open(path, "wb") as f:
        for n in S.ESCAPE_LENGTHS:
            for name, a in S.escape_contents(n).items():
                data = a.tobytes()
                want, _ = S.escape_restated(data)
                for seg in S.escape_segmentations(a, n):
                    cnt, at = [], 0
                    for s in seg:
                        cnt.append(S.escape_restated(data[at:at + s])[1]); at += s
                    f.write(np.array([n, len(seg), len(want)] + list(seg) + cnt, np.uint32).tobytes()); f.write(data); f.write(want)
                    n_rec += 1
        f.write(np.zeros(3, np.uint32).tobytes())
    print(n_rec, "escape records ->", path, os.path.getsize(path), "bytes")
else:
    key, picture, path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    c = U.slice_cases()[key]
    parts, levels, sao, rec = S.cpu_final_picture(c, picture)
    units = S.split_units(U.load_fixture()[key + "/bin"].tobytes())
    first = [k for k, (_, _, t) in enumerate(units) if t < 32][picture]      # the picture's slice NAL unit: its access unit runs from the parameter sets (picture 0) to its SEI
    want = b"".join(u for _, u, _ in units[(0 if picture == 0 else first):first + 2])
    p = S.stream_params(c, picture, 1)
    head = np.array([c["W"], c["H"], c["bd"], p.slice.qp, p.slice.slice_type, p.slice.wpp, p.slice.plain_intra, p.slice.sao_luma, p.slice.sao_chroma, p.slice.mi_size,
                     p.poc, p.parameter_sets, p.hash, parts.shape[0], 0 if sao is None else 1, len(want)], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes()); f.write(parts.tobytes()); f.write(np.ascontiguousarray(levels, np.int32).tobytes())
        if sao is not None: f.write(sao.tobytes())
        for a in rec: f.write(np.ascontiguousarray(a, np.int16).tobytes())
        f.write(want)
    print(key, picture, "->", path, os.path.getsize(path), "bytes")
