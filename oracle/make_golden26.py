#!/usr/bin/env python3
"""oracle/make_golden26.py -- TEST INFRASTRUCTURE.  Goldens of a wavefront picture whose right and bottom CTUs are partial, made by the reference encoder in the build container.

The picture is 432x184, seed 3: 6 full CTU columns + one 48 wide, 2 full CTU rows + one 56 tall -- the remainders of bench.py's 7728x5368 frame -- in 21 CTUs, as many as the
448x192 golden; seven columns are the narrowest at which a lag-5 wavefront is not raster order.  Two runs of the shim encoder with its observers on (oracle/make_golden19.py),
both with --WaveFrontSynchro=1 and one substream per CTU row:
  432x184_seed3_wpp        hoputil.lenslet(W, H, 16, 3), --MIsize=16
  432x184_seed3_mi15_wpp   hoputil.lenslet(W, H, 15, 3), --MIsize=15
Written to tests/golden/encoder_spine_ragged.npz in the layout of encoder_spine.npz (<key>/cost, /bits, /dist, /parts, /trace) plus, per run, the reference's reconstruction
BEFORE the loop filters as <key>/rec_y, /rec_cb, /rec_cr (int16): rec.yuv of a second run with --DeblockingFilterControlPresent=1 --LoopFilterDisable=1 --SAO=0, taken
only when that run's candidate trace and per-CTU cost / bits / dist / partition data are byte-identical to the first run's (the filters run after the CTU loop of an
all-intra picture and move no decision); the script asserts it.  Should the assertion ever fail, `make_golden26.py --cpu-rec` stores the reconstruction of the spine over
the CPU restatement (oracle/libhop_spine_cpu.so, lag 0) instead; <key>/rec_source says which one the file holds.
Needs /root/reference (build container)."""
import os, sys, tempfile, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from spine_check import run_reference, read_ctu_trace, run_spine  # noqa: E402

W, H, SEED = 432, 184, 3
RUNS = [("432x184_seed3_wpp", 16), ("432x184_seed3_mi15_wpp", 15)]      # key, lenslet pitch = --MIsize
# the second run: no deblocking, no SAO.  (--LoopFilterDisable reaches the slice only where the PPS carries the deblocking controls, TLibEncoder/TEncSlice.cpp:536-541: without
# --DeblockingFilterControlPresent=1 the picture is deblocked all the same)
NO_FILTERS = ("--DeblockingFilterControlPresent=1", "--LoopFilterDisable=1", "--SAO=0")


def reference(mi, extra=(), tries=4):
    """-> input planes, candidate trace (bytes), per-CTU records, rec.yuv (bytes).  (A run the encoder's out-of-buffer GT search reads kill -- make_golden24.py -- is repeated.)"""
    for k in range(tries):
        with tempfile.TemporaryDirectory() as td:
            try:
                Y, Cb, Cr, _ = run_reference(W, H, SEED, False, td, mi=mi, wpp=True, pitch=mi, extra=extra)
            except AssertionError:
                if k + 1 == tries: raise
                continue
            return (Y, Cb, Cr), open(os.path.join(td, "best.txt"), "rb").read(), read_ctu_trace(os.path.join(td, "ctu.bin")), open(os.path.join(td, "rec.yuv"), "rb").read()


def main():
    out = {}
    for key, mi in RUNS:
        (Y, Cb, Cr), text, ctu, _ = reference(mi)
        _, text2, ctu2, rec2 = reference(mi, extra=NO_FILTERS)
        same = text == text2 and ctu.tobytes() == ctu2.tobytes()
        if same:
            assert len(rec2) == W * H * 3 // 2, (key, len(rec2))
            r = np.frombuffer(rec2, np.uint8).astype(np.int16)
            rec = [r[:W * H].reshape(H, W), r[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), r[W * H * 5 // 4:].reshape(H // 2, W // 2)]
            source = "reference encoder, " + " ".join(NO_FILTERS) + " (decisions identical to the run with the filters)"
        else:                                                    # make_golden26.py --cpu-rec: only after this assertion has been seen to fail
            assert "--cpu-rec" in sys.argv, (key, " ".join(NO_FILTERS) + " changed the candidate trace or the per-CTU data")
            with tempfile.TemporaryDirectory() as td:
                rec = run_spine(W, H, Y, Cb, Cr, os.path.join(td, "mine.txt"), mi=mi, wpp_lag=0)[5]
            source = "spine over the CPU restatement, lag 0"
        out[key + "/cost"] = ctu["cost"].astype(np.float64); out[key + "/bits"] = ctu["bits"].astype(np.uint32); out[key + "/dist"] = ctu["dist"].astype(np.uint32)
        out[key + "/parts"] = ctu["p"].astype(np.int16)
        out[key + "/trace"] = np.frombuffer(zlib.compress(text, 9), np.uint8)
        out[key + "/rec_y"], out[key + "/rec_cb"], out[key + "/rec_cr"] = (np.ascontiguousarray(p, np.int16) for p in rec)
        out[key + "/rec_source"] = np.frombuffer(source.encode(), np.uint8)
        print(key, len(ctu), "CTUs", text.count(b"\n"), "candidates; reconstruction:", source, flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "encoder_spine_ragged.npz"), **out)


if __name__ == "__main__":
    main()
