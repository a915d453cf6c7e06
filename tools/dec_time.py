#!/usr/bin/python3
"""tools/dec_time.py [rows [repeats]] -- time hop_decode_frame on the bench geometry's top rows (7728 wide, synthetic lenslet of pitch 15, seed 2 like bench.py, coded by
hop_encode_frame with --MIsize=15 at wavefront lag 8; rows: 8 or 16 CTU rows).  Both schedules after a warm-up, each `repeats` times, device-synchronised (hop_decode_frame
returns after hop_sync); one JSON line: the decode rate in CTU/s (median, min, max over the repeats), levels against CTUs, launches, and whether the two schedules'
reconstructions (and SS references) are equal to each other and to the encoder's."""
import importlib.util, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hoputil import lenslet
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H = 7728, 64 * rows
Y, Cb, Cr = lenslet(W, H, 15, 2)
enc = hp.Context(W, H, slots=48); enc.upload_orig(Y, Cb, Cr)          # candidate slots as bench.py codes the frame (the result does not depend on them)
t0 = time.time()
parts = enc.encode_frame(32, 15, 0, None, wpp=1, wavefront_lag=8)[3]
enc_s = time.time() - t0
levels = enc.levels_download()
want = [enc.recon_download(c) for c in range(3)] + [enc.ssref_download(c) for c in range(3)]
dec = hp.Context(W, H)
n = parts.shape[0]
out = {"W": W, "H": H, "ctus": n, "encode_s": round(enc_s, 2), "repeats": reps}
got = {}
for schedule, name in ((0, "levels"), (1, "raster")):
    lv, nl = hp.decode_schedule(W, H, parts, schedule)
    dec.decode_frame(parts, levels, qp=32, schedule=schedule)          # warm-up (code objects, scratch)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dec.decode_frame(parts, levels, qp=32, schedule=schedule)      # synchronous: returns after the stream has drained
        ts.append(time.perf_counter() - t0)
    got[name] = [dec.recon_download(c) for c in range(3)] + [dec.ssref_download(c) for c in range(3)]
    rates = sorted(n / t for t in ts)
    out[name] = {"launches": nl, "ctu_per_s_median": round(statistics.median(rates), 1), "ctu_per_s_min": round(rates[0], 1), "ctu_per_s_max": round(rates[-1], 1),
                 "ms_median": round(1e3 * statistics.median(ts), 2)}
out["levels_vs_ctus"] = [out["levels"]["launches"], n]
out["schedules_equal"] = all(np.array_equal(a, b) for a, b in zip(got["levels"], got["raster"]))
out["equal_to_encoder"] = all(np.array_equal(a, b) for a, b in zip(got["levels"], want))
print(json.dumps(out))
