#!/usr/bin/python3
"""tools/walk_stamps.py [--out profiles/walk_stamps.json] [--quant-mode RDOQ,RDOQTS] | --show profiles/walk_stamps.json -- where thread 0 of a candidate walk's workgroup spends its cycles, stage by stage ("Stage stamps").

Runs in the DIAGNOSTIC build: HOP_LIB=hevc-hop_amd/libhophip_stamps.so (taken if HOP_LIB is unset; the product library refuses hop_walk_stamps_read).  The cases are
tests/test_gpu_walk_codegen.py's (_case / _run, imported): inter 8x8 / 16x16 / 32x32, intra 8x8 NxN, intra 16x16, noisy content, n = 1 and n = 25 candidates of the class (the
breadth of bench.py's batches); then one wavefront encode of the 448x192 --MIsize=15 picture of the stream tests, for the shares under a real mix of candidates.
Per kernel and class it prints each stage's share of the workgroups' timelines and its cycles per visit.  The instrument's own cost is NOT subtracted: hop_walk_stamps_probe
measures it (two stamps back to back; a whole stage boundary), and the column `stamp` says how much of a stage's cycles its boundaries can account for at that price.
The numbers are shares of a fenced, slower build's timeline -- not run times of the product.
--quant-mode 0,0 runs every context of the pass under hop_ctx_set_quant_mode { 0, 0 } (profiles/walk_stamps_rdoq0.json): what is left on the serial lane without RDOQ."""
import argparse
import datetime
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
os.environ.setdefault("HOP_LIB", hp.STAMPS_LIB_PATH)
import test_gpu_walk_codegen as wc  # noqa: E402
from hoputil import lenslet  # noqa: E402

CLASSES = [("inter", 3, 0), ("inter", 4, 0), ("inter", 5, 0), ("intra", 3, 1), ("intra", 4, 0)]
BREADTHS = (1, 25)


def rows_of(ctl, names, only=None):
    """the table's rows that hold something: [{kernel, log2_cu, nxn, workgroups, cycles, ..., stages: {name: {cycles, visits}}}]"""
    out = []
    for k, kn in enumerate(hp.HOP_WSK_NAMES):
        for lg in (3, 4, 5, 6):
            for nxn in (0, 1):
                if only is not None and (lg, nxn) != only: continue
                cyc, vis, tot = ctl.walk_stamps(k, lg, nxn)
                if not tot["workgroups"]: continue
                out.append(dict(kernel=kn, log2_cu=lg, nxn=nxn, **tot, stages={names[s]: {"cycles": int(cyc[s]), "visits": int(vis[s])} for s in range(hp.HOP_WS_COUNT)}))
    return out


def show(title, rows, probe):
    print("\n== %s ==" % title)
    for r in rows:
        us = r["realtime_ticks"] * 0.01 / r["workgroups"]
        print("%-13s %2dx%-2d%s  %6d workgroups, %10.0f cycles and %8.1f us each (longest %.1f us)" % (r["kernel"], 1 << r["log2_cu"], 1 << r["log2_cu"], " NxN" if r["nxn"] else "    ",
              r["workgroups"], r["cycles"] / r["workgroups"], us, r["max_realtime_ticks"] * 0.01))
        for name, s in sorted(r["stages"].items(), key=lambda kv: -kv[1]["cycles"]):
            if not s["visits"]: continue
            print("    %-13s %5.1f %%  %9d visits  %9.0f cycles / visit   stamp <= %4.1f %% of it" % (name, 100.0 * s["cycles"] / r["cycles"], s["visits"], s["cycles"] / s["visits"],
                  100.0 * min(1.0, s["visits"] * probe["mark_cycles"] / max(1, s["cycles"]))))


def show_mix(rows):
    """the encode's rows folded: per kernel over all classes, and all walk kernels together -- each stage's share of the summed timelines"""
    names = list(rows[0]["stages"])
    print("\n== the same encode, classes folded: share of all walk timelines, then %% per stage ==\n%-22s %s" % ("", " ".join("%8s" % n.replace("LEAF_", "L_").replace("NODE_", "N_") for n in names)))
    everything = sum(r["cycles"] for r in rows)
    for kn in list(hp.HOP_WSK_NAMES) + [None]:
        sel = [r for r in rows if kn is None or r["kernel"] == kn]
        tot = sum(r["cycles"] for r in sel)
        if not tot: continue
        print("%-13s %6.1f %% %s" % (kn or "all walks", 100.0 * tot / everything, " ".join("%8.1f" % (100.0 * sum(r["stages"][n]["cycles"] for r in sel) / tot) for n in names)))


def report(result):
    probe, probe0 = result["probe"], result["probe_at_start"]
    print("%s, %s, %s" % (result["date"], result["library"], result["version"]))
    print("stamp: two back to back %d cycles; a stage boundary (stamp + bookkeeping) %d cycles; in-kernel clock %.0f MHz (%d cycles in %d ticks of 100 MHz; at the start %.0f MHz)" %
          (probe["stamp_cycles"], probe["mark_cycles"], probe["clock_mhz"], probe["span_cycles"], probe["span_realtime_ticks"], probe0["clock_mhz"]))
    for c in result["classes"]: show("%s, n = %d, %s" % (c["class"], c["n"], c["content"]), c["rows"], probe)
    show("hop_encode_frame %s: %d CTUs, %d candidates" % (result["encode"]["picture"], result["encode"]["ctus"], result["encode"]["candidates"]), result["encode"]["rows"], probe)
    show_mix(result["encode"]["rows"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_stamps.json"))
    ap.add_argument("--show", metavar="JSON", help="print the tables of an earlier run's record and measure nothing")
    ap.add_argument("--quant-mode", metavar="RDOQ,RDOQTS", help="hop_ctx_set_quant_mode for every context of the pass, e.g. 0,0")
    a = ap.parse_args()
    if a.quant_mode:
        mode = tuple(int(v) for v in a.quant_mode.split(","))
        class ModeContext(hp.Context):
            def __init__(self, *args, **kw):
                super().__init__(*args, **kw)
                self.set_quant_mode(mode[0], mode[1], 0)
        hp.Context = ModeContext
    if a.show:
        with open(a.show) as f: report(json.load(f))
        return
    wc.PICS = max(BREADTHS)                                              # (a candidate per picture of the stack)
    import torch
    torch.zeros(1, device="cuda")                                       # (_run hands torch tensors to the library: torch's HIP runtime comes up first, as tests/conftest.py has it)
    ctl = hp.Context(64, 64)
    names = hp.walk_stamps_stage_names(ctl.L)
    probe0 = ctl.walk_stamps_probe()
    result = {"date": datetime.date.today().isoformat(), "library": os.path.basename(os.environ["HOP_LIB"]), "version": ctl.L.hop_version().decode(), "quant_mode": a.quant_mode or "1,1", "classes": [], "encode": None}
    for cls in CLASSES:
        for n in BREADTHS:
            wc._run(hp, cls, n, "noisy", {})                              # (once unmeasured: module load, first-touch of the work areas)
            wc._runs.pop((cls, n, "noisy", (), None))
            ctl.walk_stamps_reset()
            wc._run(hp, cls, n, "noisy", {})
            rows = rows_of(ctl, names, only=(cls[1], cls[2]))
            result["classes"].append({"class": wc._ident(cls), "n": n, "content": "noisy", "rows": rows})
    # one wavefront encode: 448x192, --MIsize=15, seed 3, candidate slots on, lag 2 (tests/test_gpu_exact_wavefront.py's picture)
    W, H = 448, 192
    ctx = hp.Context(W, H, slots=48)
    ctx.upload_orig(*lenslet(W, H, 15, 3))
    ctl.walk_stamps_reset()
    cost, bits, dist, parts, nc = ctx.encode_frame(32, 15, 0, None, wpp=1, wavefront_lag=2)
    result["encode"] = {"picture": "448x192_seed3_mi15_wpp", "ctus": int(len(cost)), "candidates": int(nc), "rows": rows_of(ctl, names)}
    ctx.close()
    probe = ctl.walk_stamps_probe()                                      # (right behind the work: the clock the stamps above counted in)
    result["probe"] = probe; result["probe_at_start"] = probe0
    ctl.close()
    report(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f: json.dump(result, f, indent=1)
    print("\nwrote", a.out)


if __name__ == "__main__":
    main()
