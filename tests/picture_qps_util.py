"""Helpers of the per-picture-QP tests (tests/test_picture_qps_cpu.py, tests/test_gpu_picture_qps.py): the streams of tests/golden/stream_qps.npz
(tools/make_golden_qps.py) -- the unmodified reference encoder's bitstreams of two slice-data cases at QPs other than 32 -- next to the QP-32 stream of the same case in
tests/golden/slice_data.npz.

The reference switches neither slice SAO flag at any of these QPs (the tool asserts it), so no QP had to be moved from the four rate points 22 / 27 / 32 / 37."""
import os

import numpy as np

import slicedata_util as U

FIXTURE = os.path.join(U.ROOT, "tests", "golden", "stream_qps.npz")
QPS = {"192x128_wpp": (22, 27, 32, 37), "136x72_plain8": (22, 32, 37)}      # per case, rising; 32 is slice_data.npz's
STREAMS = [(key, qp) for key, qps in QPS.items() for qp in qps]
CASES = U.slice_cases()


def stream(key, qp):
    """the whole .bin (one access unit) of the case coded at qp"""
    if qp == 32:
        return U.load_fixture()[key + "/bin"].tobytes()
    return np.load(FIXTURE)["%s/q%d/bin" % (key, qp)].tobytes()


def case_at(key, qp):
    """the slice-data case with its QP replaced: what stream_util.cpu_final_picture, slicedata_util.params_of and stream_util.stream_params read"""
    c = dict(CASES[key])
    c["qp"] = qp
    if c["plain"]:
        c["plain"] = (c["plain"][0], qp)
    return c
