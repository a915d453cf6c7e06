#!/usr/bin/python3
"""tools/entropy_time.py [rows [repeats]] -- time hop_slice_data_write beside the transfer it makes unnecessary, hop_levels_download, on the same build and pictures:
the 448x192 picture of the goldens (448x192_seed3_mi15_wpp: seed 3, pitch 15, --MIsize=15, WaveFrontSynchro) and the bench geometry's top rows (7728 wide, seed 2,
lag 8, candidate slots as bench.py; rows: 8 CTU rows), the setup tools/dec_time.py uses.  Each picture is coded, deblocked and SAO-decided by the library; then, after a
warm-up, `repeats` calls of each: the writer's context pass and coding pass by HIP events (hop_profile_*: HOP_K_ENTROPY_CTX, HOP_K_ENTROPY), the whole call and the download by the host clock,
device-synchronised (both entries return after the stream has drained).  One JSON line: medians in ms, the launches, the bytes either way."""
import importlib.util, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hoputil import lenslet
from slicedata_util import sao_lambdas
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out = {"repeats": reps}
for name, W, H, seed, lag, slots in (("448x192_seed3_mi15_wpp", 448, 192, 3, 5, 16), ("7728x%d_band" % (64 * rows), 7728, 64 * rows, 2, 8, 48)):
    Y, Cb, Cr = lenslet(W, H, 15, seed)
    ctx = hp.Context(W, H, slots=slots); ctx.upload_orig(Y, Cb, Cr)
    parts = ctx.encode_frame(32, 15, 0, None, wpp=1, wavefront_lag=lag)[3]
    ctx.deblock_frame(parts, 32)
    sao = ctx.sao_frame(sao_lambdas(32), 3, 32, int(ctx.rd_fraction_download()[-1]))
    write = lambda: ctx.slice_data_write(parts, None, sao, 32, 3, 1, 0, mi_size=15)
    data, sizes, nsub = write()                                        # warm-up (code objects, scratch)
    ctx.levels_download()
    ctx.profile(on=True)
    t_ctx, t_code, t_call, t_down = [], [], [], []
    for _ in range(reps):
        ctx.profile(reset=True)
        t0 = time.perf_counter(); again = write(); t_call.append(time.perf_counter() - t0)
        assert again[0] == data
        t_ctx.append(ctx.profile(read=hp.HOP_K_ENTROPY_CTX)[1]); t_code.append(ctx.profile(read=hp.HOP_K_ENTROPY)[1])
        t0 = time.perf_counter(); lv = ctx.levels_download(); t_down.append(time.perf_counter() - t0)
    med = lambda v, k=1.0: round(k * statistics.median(v), 3)
    out[name] = {"ctus": int(parts.shape[0]), "substreams": int(nsub), "slice_data_bytes": len(data), "launches": 3, "context_pass_ms": med(t_ctx), "coding_pass_ms": med(t_code),
                 "whole_call_ms": med(t_call, 1e3), "levels_download_ms": med(t_down, 1e3), "levels_bytes": int(lv.nbytes)}
    ctx.close()
print(json.dumps(out))
