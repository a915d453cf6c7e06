#!/usr/bin/python3
"""tools/parse_time.py [rows [repeats]] -- time hop_slice_data_parse beside the writer's coding pass and hop_decode_frame, the method and the pictures of
tools/entropy_time.py: the 448x192 picture of the goldens (448x192_seed3_mi15_wpp) and the bench geometry's top rows (7728 wide, seed 2, lag 8; rows: 8 CTU rows).  Each
picture is coded, deblocked, SAO-decided and written by the library; then, after a warm-up, `repeats` calls of each: the parser's launches by HIP events (hop_profile_*:
HOP_K_PARSE; the writer's HOP_K_ENTROPY_CTX / HOP_K_ENTROPY likewise), the whole calls by the host clock, device-synchronised.  The parsed data must be what the picture
decodes from.  One JSON line: medians in ms, the launches, and the parser's ms per CTU of the serial lane -- a diagonal launch lasts as long as one CTU of its slowest
row, so this is the summed kernel time over the launches."""
import importlib.util, json, os, statistics, sys, time
import numpy as np
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
    levels = ctx.levels_download()
    ctx.deblock_frame(parts, 32)
    sao = ctx.sao_frame(sao_lambdas(32), 3, 32, int(ctx.rd_fraction_download()[-1]))
    write = lambda: ctx.slice_data_write(parts, None, sao, 32, 3, 1, 0, mi_size=15)
    data, sizes, nsub = write()
    parse = lambda: ctx.slice_data_parse(data, sizes, qp=32, slice_type=3, wpp=1, plain_intra=0, sao_luma=1, sao_chroma=1, mi_size=15)
    got = parse()                                                       # warm-up (code objects, scratch), and the check
    assert np.array_equal(got[1], levels) and got[2].tobytes() == sao.tobytes() and np.array_equal(got[0]["mv"], parts["mv"]) and np.array_equal(got[0]["cbf"], parts["cbf"])
    dec = hp.Context(W, H)
    dec.decode_frame(got[0], got[1], qp=32)                             # warm-up
    ctx.profile(on=True)
    t_parse, t_pcall, t_ctx, t_code, t_wcall, t_dec, launches = [], [], [], [], [], [], 0
    for _ in range(reps):
        ctx.profile(reset=True)
        t0 = time.perf_counter(); write(); t_wcall.append(time.perf_counter() - t0)
        t_ctx.append(ctx.profile(read=hp.HOP_K_ENTROPY_CTX)[1]); t_code.append(ctx.profile(read=hp.HOP_K_ENTROPY)[1])
        t0 = time.perf_counter(); parse(); t_pcall.append(time.perf_counter() - t0)
        launches, ms, _ = ctx.profile(read=hp.HOP_K_PARSE); t_parse.append(ms)
        t0 = time.perf_counter(); dec.decode_frame(got[0], got[1], qp=32); t_dec.append(time.perf_counter() - t0)
    med = lambda v, k=1.0: round(k * statistics.median(v), 3)
    out[name] = {"ctus": int(parts.shape[0]), "substreams": int(nsub), "slice_data_bytes": len(data), "parse_launches": launches, "parse_kernels_ms": med(t_parse),
                 "parse_whole_call_ms": med(t_pcall, 1e3), "parse_ms_per_ctu_of_a_row": round(statistics.median(t_parse) / launches, 4),
                 "write_context_pass_ms": med(t_ctx), "write_coding_pass_ms": med(t_code), "write_whole_call_ms": med(t_wcall, 1e3), "decode_frame_ms": med(t_dec, 1e3)}
    ctx.close(); dec.close()
print(json.dumps(out))
