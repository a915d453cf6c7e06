#!/usr/bin/python3
"""tools/stream_read_time.py [repeats] -- time the stream read back beside its parts, on the 448x192 wavefront stream of the goldens (448x192_seed3_mi15_wpp, the
reference encoder's own bytes), with the method of tools/stream_time.py: a warm-up, then `repeats` (default five) calls of each, medians in ms:
  - the three unescape launches of hop_access_unit_read by HIP events (hop_profile_*: HOP_K_UNESCAPE);
  - hop_access_unit_decode whole, by the host clock (it returns after the stream has drained), and its parts alone: hop_access_unit_read, hop_slice_data_parse on the
    reader's RBSP, hop_decode_frame, hop_deblock_frame, hop_sao_apply, hop_picture_hash (MD5);
  - hop_rbsp_unescape on the escaped slice data (upload, launches, download) beside the host loop hop_rbsp_unescape_host on the same bytes.
One JSON line.  No claim or threshold hangs on these numbers."""
import importlib.util, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U
spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py")); hp = importlib.util.module_from_spec(spec); spec.loader.exec_module(hp)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KEY = "448x192_seed3_mi15_wpp"


def timed(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter(); r = fn(); t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3), r


c = U.slice_cases()[KEY]
au = hp.annexb_access_units(U.load_fixture()[KEY + "/bin"].tobytes())[0]
ctx = hp.Context(c["W"], c["H"])
info, match, parts, levels, sao = ctx.access_unit_decode(au)                # warm-up (code objects, scratch)
assert match == [1, 1, 1]
rinfo, rbsp, sizes, digest = ctx.access_unit_read(au)
s = info.params.slice
kw = dict(qp=s.qp, slice_type=s.slice_type, wpp=s.wpp, plain_intra=s.plain_intra, sao_luma=s.sao_luma, sao_chroma=s.sao_chroma, mi_size=s.mi_size)
vcl = [u for u in U.nal_units(au) if ((u[0] >> 1) & 0x3F) < 32][0]
escaped = vcl[info.header_bytes - 2:]                                       # two bytes of lookback, then the escaped substreams
seg = [len(escaped) - 2]
assert ctx.rbsp_unescape(escaped, seg, lookback=2)[0] == hp.rbsp_unescape_host(escaped, seg, lookback=2, lib=ctx.L)[0] == rbsp
recon = ctx.sao_reconstruct_params(sao)
r = {"repeats": reps, "stream": KEY, "access_unit_bytes": len(au), "slice_data_bytes": len(rbsp), "substreams": int(info.n_substreams), "ctus": int(parts.shape[0])}
r["access_unit_decode_ms"] = timed(lambda: ctx.access_unit_decode(au, want_outputs=False), reps)[0]
r["access_unit_read_ms"] = timed(lambda: ctx.access_unit_read(au), reps)[0]
r["slice_data_parse_ms"] = timed(lambda: ctx.slice_data_parse(rbsp, sizes, **kw), reps)[0]
r["decode_frame_ms"] = timed(lambda: ctx.decode_frame(parts, levels, qp=s.qp, plain_intra=s.plain_intra), reps)[0]
r["deblock_frame_ms"] = timed(lambda: ctx.deblock_frame(parts, s.qp), reps)[0]
r["sao_apply_ms"] = timed(lambda: ctx.sao_apply(recon), reps)[0]
r["picture_hash_md5_ms"] = timed(lambda: ctx.picture_hash(1), reps)[0]
ctx.profile(on=True)
t_une = []
for _ in range(reps):
    ctx.profile(reset=True); ctx.access_unit_read(au); t_une.append(ctx.profile(read=hp.HOP_K_UNESCAPE))
ctx.profile(on=False)
r["unescape_launches_ms"] = round(statistics.median(t[1] for t in t_une), 4); r["unescape_launch_groups"] = t_une[0][0]
r["rbsp_unescape_device_call_ms"] = timed(lambda: ctx.rbsp_unescape(escaped, seg, lookback=2), reps)[0]
r["rbsp_unescape_host_loop_ms"] = timed(lambda: hp.rbsp_unescape_host(escaped, seg, lookback=2, lib=ctx.L), reps)[0]
ctx.close()
print(json.dumps(r))
