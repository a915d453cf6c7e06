#!/usr/bin/python3
"""tools/stream_time.py [rows [repeats]] -- time the outer layer of the stream beside what it replaces, on the pictures of tools/entropy_time.py: the 448x192 picture of
the goldens (448x192_seed3_mi15_wpp) and the bench geometry's top rows (7728 wide, seed 2, lag 8; rows: 8 CTU rows).  Each picture is coded, deblocked and SAO-decided by
the library; then, after a warm-up, `repeats` calls of each:
  - hop_access_unit_write (MD5 and checksum) and hop_slice_data_write alone, by the host clock (both return after the stream has drained);
  - the escape launches of the access unit (count over the substreams, then count / scan / scatter over header + substreams) by HIP events (hop_profile_*: HOP_K_ESCAPE);
  - hop_rbsp_escape on the downloaded slice data (upload, launches, download) and the host loop hop_rbsp_escape_host on the same bytes;
  - the checksum pass (HOP_K_PICHASH, and the whole hop_picture_hash call) beside the download of the three planes it avoids, and the MD5 of hop_picture_hash.
One JSON line: medians in ms."""
import importlib.util, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hoputil import lenslet
from slicedata_util import sao_lambdas
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out = {"repeats": reps}


def timed(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter(); r = fn(); t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3), r


for name, W, H, seed, lag, slots in (("448x192_seed3_mi15_wpp", 448, 192, 3, 5, 16), ("7728x%d_band" % (64 * rows), 7728, 64 * rows, 2, 8, 48)):
    Y, Cb, Cr = lenslet(W, H, 15, seed)
    ctx = hp.Context(W, H, slots=slots); ctx.upload_orig(Y, Cb, Cr)
    parts = ctx.encode_frame(32, 15, 0, None, wpp=1, wavefront_lag=lag)[3]
    ctx.deblock_frame(parts, 32)
    sao = ctx.sao_frame(sao_lambdas(32), 3, 32, int(ctx.rd_fraction_download()[-1]))
    kw = dict(qp=32, slice_type=3, wpp=1, plain_intra=0, mi_size=15)
    au = lambda h: ctx.access_unit_write(parts, None, sao, hash=h, **kw)
    sd = lambda: ctx.slice_data_write(parts, None, sao, 32, 3, 1, 0, mi_size=15)
    data, sizes, nsub = sd(); unit = au(1)[0]; au(3); au(0)                  # warm-up (code objects, scratch)
    esc_dev = lambda: ctx.rbsp_escape(data, sizes)
    esc_host = lambda: hp.rbsp_escape_host(data, sizes, lib=ctx.L)
    assert esc_dev()[0] == esc_host()[0]
    r = {"ctus": int(parts.shape[0]), "substreams": int(nsub), "slice_data_bytes": len(data), "access_unit_bytes": len(unit)}
    r["slice_data_write_ms"] = timed(sd, reps)[0]
    r["access_unit_write_nohash_ms"] = timed(lambda: au(0), reps)[0]
    r["access_unit_write_md5_ms"] = timed(lambda: au(1), reps)[0]
    r["access_unit_write_checksum_ms"] = timed(lambda: au(3), reps)[0]
    ctx.profile(on=True)
    t_esc = []
    for _ in range(reps):
        ctx.profile(reset=True); au(0); t_esc.append(ctx.profile(read=hp.HOP_K_ESCAPE))
    r["escape_launches_ms"] = round(statistics.median(t[1] for t in t_esc), 4); r["escape_launch_groups"] = t_esc[0][0]
    t_sum = []
    for _ in range(reps):
        ctx.profile(reset=True); ctx.picture_hash(3); t_sum.append(ctx.profile(read=hp.HOP_K_PICHASH)[1])
    r["checksum_pass_ms"] = round(statistics.median(t_sum), 4)
    ctx.profile(on=False)
    r["rbsp_escape_device_call_ms"] = timed(esc_dev, reps)[0]
    r["rbsp_escape_host_loop_ms"] = timed(esc_host, reps)[0]
    r["picture_hash_checksum_call_ms"] = timed(lambda: ctx.picture_hash(3), reps)[0]
    r["picture_hash_md5_call_ms"] = timed(lambda: ctx.picture_hash(1), reps)[0]
    r["three_planes_download_ms"] = timed(lambda: [ctx.recon_download(k) for k in range(3)], reps)[0]
    out[name] = r
    ctx.close()
print(json.dumps(out))
