#!/usr/bin/python3
"""tools/qp_sweep_time.py [--content small|band|both] [--repeats 3] -- time the four rate points of one frame (QP 22 / 27 / 32 / 37, BASELINE.md config 4's set).

  base    one context, hop_encode_frame four times, one QP after the other (the only way before hop_ctx_set_picture_qps)
  stack   a stacked context of four copies of the picture with the table set, ONE hop_encode_frame
Content: `small` the 448x192 picture of the slice-data case 448x192_seed3_mi15_wpp (21 CTUs); `band` the top 7728x128 band of bench.py's frame (242 CTUs).  Same
wavefront lag (5), candidate slots (16), HOP_SPINE_STREAMS / HOP_SPINE_SETS (the environment's) and micro-image size (15) in both paths.

Method, as tools/stack_decode_time.py: a warm-up of each path, then `repeats` timed passes with the paths alternating; whole calls by the host clock (hop_encode_frame
returns after its streams have drained); medians.  Every pass checks its per-CTU costs and partition data against the other path's: picture k of the stack must be the
base's encode at QP k, bit for bit.  The warm-up passes run the whole chain (deblocking, SAO -- hop_sao_frame in the base, hop_sao_frame_pictures in the stack --,
hop_access_unit_write, hop_psnr), compare the access units of the two paths byte for byte and give the rate points themselves: bits and PSNR per QP.
Decode leg: the four access units through hop_access_unit_decode four times on one context against one hop_access_units_decode into a stack of four, timed the same
way, every pass checking all hashes.

One process; run it under `timeout`.  One JSON line per content, the same into profiles/qp_sweep.json, then the table in markdown."""
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
QPS, MI, LAG, SLOTS = [22, 27, 32, 37], 15, 5, 16
WRITE = dict(slice_type=3, wpp=1, plain_intra=0, mi_size=MI)


def content(name):
    if name == "small":
        return 448, 192, lenslet(448, 192, 15, 3)
    bench = load("bench", os.path.join(ROOT, "bench.py"))
    Y, Cb, Cr = bench.frame_planes(7728, 5368, 2)
    return 7728, 128, (np.ascontiguousarray(Y[:128]), np.ascontiguousarray(Cb[:64]), np.ascontiguousarray(Cr[:64]))


def split(data, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return [data[edges[k]:edges[k + 1]] for k in range(len(sizes))]


def base_encode(ctx):
    """[(cost, parts)] per QP and the seconds of the four hop_encode_frame calls"""
    out, s = [], 0.0
    for qp in QPS:
        t0 = time.perf_counter(); r = ctx.encode_frame(qp, MI, 0, None, wpp=1, wavefront_lag=LAG); s += time.perf_counter() - t0
        out.append((r[0], r[3]))
    return out, s


def stack_encode(ctx):
    t0 = time.perf_counter(); r = ctx.encode_frame(32, MI, 0, None, wpp=1, wavefront_lag=LAG); s = time.perf_counter() - t0
    n = len(r[0]) // len(QPS)
    return [(r[0][k * n:(k + 1) * n], r[3][k * n:(k + 1) * n]) for k in range(len(QPS))], s


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes() for x, y in zip(a, b))


def base_chain(ctx):
    """the whole chain per QP on one context: access units, bits, PSNR"""
    aus, psnr = [], []
    for qp in QPS:
        parts = ctx.encode_frame(qp, MI, 0, None, wpp=1, wavefront_lag=LAG)[3]
        ctx.deblock_frame(parts, qp)
        sao = ctx.sao_frame(U.sao_lambdas(qp), 3, qp, int(ctx.rd_fraction_download()[-1]))
        aus.append(ctx.access_unit_write(parts, None, sao, qp=qp, hash=1, **WRITE)[0])
        psnr.append(ctx.psnr()[1][0].tolist())
    return aus, psnr


def stack_chain(ctx):
    parts = ctx.encode_frame(32, MI, 0, None, wpp=1, wavefront_lag=LAG)[3]
    ctx.deblock_frame(parts, 32)
    sao = ctx.sao_frame_pictures([(U.sao_lambdas(qp), 3, qp, 0) for qp in QPS])
    data, sizes = ctx.access_unit_write(parts, None, sao, qp=32, hash=1, **WRITE)
    return split(data, sizes), ctx.psnr()[1].tolist()


def run(name, reps):
    W, H, (Y, Cb, Cr) = content(name)
    n_ctu = ((W + 63) // 64) * ((H + 63) // 64)
    base = hp.Context(W, H, slots=SLOTS)
    base.upload_orig(Y, Cb, Cr)
    stack = hp.Context(W, H, pictures=len(QPS), slots=SLOTS)
    stack.upload_orig(stack.stack([Y] * len(QPS)), stack.stack([Cb] * len(QPS), True), stack.stack([Cr] * len(QPS), True))
    stack.set_picture_qps(QPS)
    aus, psnr = base_chain(base)                                           # warm-up of each path: code objects, work areas at their final size; the rate points
    aus_s, psnr_s = stack_chain(stack)
    assert aus == aus_s, "the access units of the two paths differ"
    assert np.allclose(psnr, psnr_s, rtol=0, atol=0), (psnr, psnr_s)
    tb, ts = [], []
    for _ in range(reps):
        rb, s = base_encode(base); tb.append(s)
        rs, s = stack_encode(stack); ts.append(s)
        assert same(rb, rs), "per-CTU costs or partition data of the two paths differ"
    base.close(); stack.close()
    # the decode leg
    one, four = hp.Context(W, H), hp.Context(W, H, pictures=len(QPS))
    db, ds = [], []
    for i in range(reps + 1):                                              # (pass 0: the warm-up)
        t0 = time.perf_counter()
        for au in aus:
            assert one.access_unit_decode(au, want_outputs=False)[1] == [1, 1, 1]
        b = time.perf_counter() - t0
        t0 = time.perf_counter()
        assert four.access_units_decode(aus, want_outputs=False)[1] == [[1, 1, 1]] * len(QPS)
        s = time.perf_counter() - t0
        if i:
            db.append(b); ds.append(s)
    one.close(); four.close()
    mb, ms, mdb, mds = (statistics.median(v) for v in (tb, ts, db, ds))
    return {"content": name, "picture": [W, H], "ctus_per_picture": n_ctu, "qps": QPS, "lag": LAG, "slots": SLOTS, "mi_size": MI, "repeats": reps,
            "streams": os.environ.get("HOP_SPINE_STREAMS"), "sets": os.environ.get("HOP_SPINE_SETS"),
            "bits": [8 * len(a) for a in aus], "psnr_y_cb_cr": [[round(v, 4) for v in p] for p in psnr],
            "base_encode_s": round(mb, 3), "base_encode_s_min_max": [round(min(tb), 3), round(max(tb), 3)], "stack_encode_s": round(ms, 3), "stack_encode_s_min_max": [round(min(ts), 3), round(max(ts), 3)],
            "base_ctu_per_s": round(len(QPS) * n_ctu / mb, 1), "stack_ctu_per_s": round(len(QPS) * n_ctu / ms, 1), "encode_base_over_stack": round(mb / ms, 2),
            "base_decode_ms": round(1e3 * mdb, 2), "stack_decode_ms": round(1e3 * mds, 2), "decode_base_over_stack": round(mdb / mds, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="both", choices=("small", "band", "both"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qp_sweep.json"))
    a = ap.parse_args()
    rows = []
    for name in (("small", "band") if a.content == "both" else (a.content,)):
        rows.append(run(name, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| content | CTUs x 4 | bits at 22 / 27 / 32 / 37 | Y-PSNR | base: 4 encodes | stack: 1 encode | base / stack | base: 4 decodes | stack: 1 decode | base / stack |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s %dx%d | %d | %s | %s | %.2f s (%.1f CTU/s) | %.2f s (%.1f CTU/s) | %.2f | %.2f ms | %.2f ms | %.2f |" % (
            r["content"], r["picture"][0], r["picture"][1], 4 * r["ctus_per_picture"], " / ".join(str(b) for b in r["bits"]), " / ".join("%.2f" % p[0] for p in r["psnr_y_cb_cr"]),
            r["base_encode_s"], r["base_ctu_per_s"], r["stack_encode_s"], r["stack_ctu_per_s"], r["encode_base_over_stack"], r["base_decode_ms"], r["stack_decode_ms"], r["decode_base_over_stack"]))


if __name__ == "__main__":
    main()
