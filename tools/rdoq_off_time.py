#!/usr/bin/python3
"""tools/rdoq_off_time.py [--content small|band|both] [--repeats 3] -- what hop_ctx_set_quant_mode gains and costs: hop_encode_frame of one picture at QP 32 with
RDOQ on (the default, {1, 1}), off ({0, 0}) and off for transform-skip units only ({1, 0}).

Content: `small` the 448x192 picture of the slice-data case 448x192_seed3_mi15_wpp (21 CTUs); `band` the top 7728x128 band of bench.py's frame (242 CTUs).  Same
wavefront lag (5), candidate slots (16), HOP_SPINE_STREAMS / HOP_SPINE_SETS (the environment's) and micro-image size (15) in every mode.

Method, as tools/qp_sweep_time.py: ONE context; a warm-up of each mode that runs the whole chain (deblocking, SAO, hop_access_unit_write, hop_psnr) and gives the mode's
bits and PSNR; then `repeats` timed hop_encode_frame calls per mode, the modes alternating; whole calls by the host clock (hop_encode_frame returns after its streams
have drained); medians with minimum and maximum.  Every timed pass checks its per-CTU costs against the warm-up's of its mode.

One process; run it under `timeout`.  One JSON line per content, the same into profiles/rdoq_off.json, then the table in markdown."""
import argparse, importlib.util, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402
from hoputil import lenslet  # noqa: E402


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path); m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


hp = load("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
QP, MI, LAG, SLOTS = 32, 15, 5, 16
MODES = [("rdoq on", (1, 1)), ("rdoq off", (0, 0)), ("rdoq on, ts off", (1, 0))]
WRITE = dict(slice_type=3, wpp=1, plain_intra=0, mi_size=MI)


def content(name):
    if name == "small":
        return 448, 192, lenslet(448, 192, 15, 3)
    bench = load("bench", os.path.join(ROOT, "bench.py"))
    Y, Cb, Cr = bench.frame_planes(7728, 5368, 2)
    return 7728, 128, (np.ascontiguousarray(Y[:128]), np.ascontiguousarray(Cb[:64]), np.ascontiguousarray(Cr[:64]))


def chain(ctx):
    """the whole chain in the context's mode: (per-CTU costs, bits of the access unit, PSNR Y / Cb / Cr)"""
    r = ctx.encode_frame(QP, MI, 0, None, wpp=1, wavefront_lag=LAG)
    ctx.deblock_frame(r[3], QP)
    sao = ctx.sao_frame(U.sao_lambdas(QP), 3, QP, int(ctx.rd_fraction_download()[-1]))
    au = ctx.access_unit_write(r[3], None, sao, qp=QP, hash=1, **WRITE)[0]
    return r[0], 8 * len(au), ctx.psnr()[1][0].tolist()


def run(name, reps):
    W, H, (Y, Cb, Cr) = content(name)
    n_ctu = ((W + 63) // 64) * ((H + 63) // 64)
    ctx = hp.Context(W, H, slots=SLOTS)
    ctx.upload_orig(Y, Cb, Cr)
    warm = {}
    for label, m in MODES:                                                  # warm-up of each mode: code objects, work areas at their final size; bits and PSNR
        ctx.set_quant_mode(m[0], m[1], 0)
        warm[label] = chain(ctx)
        print("%s: warm-up, %s: %d bits" % (name, label, warm[label][1]), file=sys.stderr, flush=True)
    t = {label: [] for label, _ in MODES}
    for _ in range(reps):
        for label, m in MODES:
            ctx.set_quant_mode(m[0], m[1], 0)
            t0 = time.perf_counter(); r = ctx.encode_frame(QP, MI, 0, None, wpp=1, wavefront_lag=LAG); t[label].append(time.perf_counter() - t0)
            assert np.array_equal(r[0], warm[label][0]), "%s: the per-CTU costs of two passes differ" % label
            print("%s: %s: %.3f s" % (name, label, t[label][-1]), file=sys.stderr, flush=True)
    ctx.close()
    row = {"content": name, "picture": [W, H], "ctus": n_ctu, "qp": QP, "lag": LAG, "slots": SLOTS, "mi_size": MI, "repeats": reps,
           "streams": os.environ.get("HOP_SPINE_STREAMS"), "sets": os.environ.get("HOP_SPINE_SETS"), "modes": {}}
    for label, m in MODES:
        med = statistics.median(t[label])
        row["modes"][label] = {"rdoq": m[0], "rdoq_ts": m[1], "encode_s": round(med, 3), "encode_s_min_max": [round(min(t[label]), 3), round(max(t[label]), 3)],
                               "ctu_per_s": round(n_ctu / med, 1), "bits": warm[label][1], "psnr_y_cb_cr": [round(v, 4) for v in warm[label][2]],
                               "rd_cost": float(np.sum(warm[label][0]))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="both", choices=("small", "band", "both"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdoq_off.json"))
    a = ap.parse_args()
    rows = []
    for name in (("small", "band") if a.content == "both" else (a.content,)):
        rows.append(run(name, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| content | CTUs | mode | hop_encode_frame, median (min .. max) | CTU/s | against RDOQ on | bits | Y-PSNR |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        on = r["modes"][MODES[0][0]]
        for label, _ in MODES:
            m = r["modes"][label]
            print("| %s %dx%d | %d | %s | %.3f s (%.3f .. %.3f) | %.1f | %.2f x | %d (%+.1f %%) | %.2f dB (%+.2f) |" % (
                r["content"], r["picture"][0], r["picture"][1], r["ctus"], label, m["encode_s"], m["encode_s_min_max"][0], m["encode_s_min_max"][1], m["ctu_per_s"],
                on["encode_s"] / m["encode_s"], m["bits"], 100.0 * (m["bits"] - on["bits"]) / on["bits"], m["psnr_y_cb_cr"][0], m["psnr_y_cb_cr"][0] - on["psnr_y_cb_cr"][0]))


if __name__ == "__main__":
    main()
