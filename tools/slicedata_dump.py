#!/usr/bin/env python3
"""tools/slicedata_dump.py <case> <out.dump> -- one fixture case of tests/slicedata_util.py as the file tools/slicedata_host_check.cpp reads: the picture coded on the CPU
(tests/slicedata_cpu.py: the RD spine over the restatement, the restated loop filter, hop_sao_decide), and as the expected bytes the slice data of the reference encoder's
own stream (tests/golden/slice_data.npz).  Build container only (the CPU spine library)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_cpu as C  # noqa: E402
import slicedata_util as U  # noqa: E402

key, path = sys.argv[1], sys.argv[2]
c = U.slice_cases()[key]
parts, levels, sao = C.cpu_picture(c, 0)
data, sizes = C.host_slice_data(c, 0)
want, _ = U.fixture_slice_data(U.load_fixture(), key, 0, len(data))
p = U.params_of(c)
head = np.array([c["W"], c["H"], c["bd"], p.qp, p.slice_type, p.wpp, p.plain_intra, p.sao_luma, p.sao_chroma, p.mi_size, parts.shape[0], 0 if sao is None else 1, len(sizes), len(want), 0, 0], np.int32)
with open(path, "wb") as f:
    f.write(head.tobytes()); f.write(parts.tobytes()); f.write(np.ascontiguousarray(levels, np.int32).tobytes())
    if sao is not None: f.write(sao.tobytes())
    f.write(np.ascontiguousarray(sizes, np.uint32).tobytes()); f.write(want)
print(key, "->", path, os.path.getsize(path), "bytes")
