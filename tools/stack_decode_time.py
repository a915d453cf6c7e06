#!/usr/bin/python3
"""tools/stack_decode_time.py [repeats] -- time the decode of n views of BASELINE config 5's geometry (624x432, WaveFrontSynchro) from their access units.

Three distinct views (synthetic lenslets of pitch 16, seeds 7, 21, 22) are coded once in a stacked context, deblocked and written by hop_access_unit_write with the
checksum SEI; n = 1, 8, 64 and 169 pictures cycle through them.
  base      one context, hop_access_unit_decode n times (what a caller had before hop_access_units_decode)
  stack     a stacked context of n pictures, one hop_access_units_decode
Per n: a warm-up of each path, then `repeats` (default 3) timed passes, base and stack alternating; whole calls by the host clock, each call returning after the stream has
drained; medians.  The parser's share (HOP_K_PARSE of hop_profile_read: summed kernel time of its launches, by HIP events) comes from one more pass of each path with
profiling on, outside the timed passes.  Every pass checks that all hashes match.  One process; run it under `timeout`.  One JSON line per n, then the table in markdown."""
import importlib.util, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hoputil import lenslet
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
W, H, QP, MI = 624, 432, 32, 16
views = [lenslet(W, H, 16, seed) for seed in (7, 21, 22)]
enc = hp.Context(W, H, pictures=len(views), slots=16)
enc.upload_orig(enc.stack([v[0] for v in views]), enc.stack([v[1] for v in views], True), enc.stack([v[2] for v in views], True))
t0 = time.time()
parts = enc.encode_frame(QP, MI, 0, None, wpp=1, wavefront_lag=5)[3]
enc_s = time.time() - t0
enc.deblock_frame(parts, QP)
data, sizes = enc.access_unit_write(parts, None, None, qp=QP, slice_type=3, wpp=1, plain_intra=0, mi_size=MI, hash=3)
enc.close()
edges = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
aus = [data[edges[k]:edges[k + 1]] for k in range(len(views))]
n_ctu = ((W + 63) // 64) * ((H + 63) // 64)
print(json.dumps({"W": W, "H": H, "ctus_per_picture": n_ctu, "views": len(views), "encode_s": round(enc_s, 2), "au_bytes": [len(a) for a in aus], "repeats": reps}), flush=True)


def run_base(ctx, units):
    for au in units:
        assert ctx.access_unit_decode(au, want_outputs=False)[1] == [1, 1, 1]


def run_stack(ctx, units):
    assert ctx.access_units_decode(units, want_outputs=False)[1] == [[1, 1, 1]] * len(units)


def parse_ms(ctx, run, units):
    ctx.profile(on=True, reset=True)
    run(ctx, units)
    launches, ms, _ = ctx.profile(read=hp.HOP_K_PARSE)
    ctx.profile(on=False)
    return launches, ms


rows = []
for n in (1, 8, 64, 169):
    units = [aus[k % len(aus)] for k in range(n)]
    base, stack = hp.Context(W, H), hp.Context(W, H, pictures=n)
    run_base(base, units); run_stack(stack, units)                         # warm-up: code objects, the scratch areas at their final size
    tb, ts = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); run_base(base, units); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); run_stack(stack, units); ts.append(time.perf_counter() - t0)
    lb, pb = parse_ms(base, run_base, units)
    ls, ps = parse_ms(stack, run_stack, units)
    base.close(); stack.close()
    mb, ms_ = statistics.median(tb), statistics.median(ts)
    r = {"n": n, "base_ms": round(1e3 * mb, 2), "base_ms_min_max": [round(1e3 * min(tb), 2), round(1e3 * max(tb), 2)], "base_parse_launches": lb, "base_parse_ms": round(pb, 2),
         "base_pictures_per_s": round(n / mb, 1), "stack_ms": round(1e3 * ms_, 2), "stack_ms_min_max": [round(1e3 * min(ts), 2), round(1e3 * max(ts), 2)],
         "stack_parse_launches": ls, "stack_parse_ms": round(ps, 2), "stack_pictures_per_s": round(n / ms_, 1), "base_over_stack": round(mb / ms_, 2)}
    rows.append(r)
    print(json.dumps(r), flush=True)
print("| n | base: total | base: parser (launches) | base: pictures/s | stack: total | stack: parser (launches) | stack: pictures/s | base / stack |")
print("|---|---|---|---|---|---|---|---|")
for r in rows:
    print("| %d | %.2f ms | %.2f ms (%d) | %.1f | %.2f ms | %.2f ms (%d) | %.1f | %.2f |" % (r["n"], r["base_ms"], r["base_parse_ms"], r["base_parse_launches"], r["base_pictures_per_s"],
                                                                                        r["stack_ms"], r["stack_parse_ms"], r["stack_parse_launches"], r["stack_pictures_per_s"], r["base_over_stack"]))
