"""GPU: the final luma pass of the intra search where it repeats the winner (rqt_intra_final_repeats, csrc/k_walk.inl).

estIntraPredQT sends a PU's best mode through the transform tree once more without bCheckFirst.  For a PU whose root transform unit cannot split (the 4x4 PUs of an NxN
8x8 CU) that is the winner's own candidate pass over again, nothing of it is kept, and the library leaves it out.  HOP_INTRA_FINAL_ALWAYS=1 runs it all the same: every
output, and the context's reconstruction planes after the call, must be the same bytes with and without it, in every form of the candidate chain -- the candidates of a PU
side by side (k_iw_*, the default), one after the other (HOP_WALK_CAND=0) and as batch steps (HOP_WALK=0: hop_launch_intra_search) -- and through hop_encode_frame."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import degenerate as dg
from hoputil import ROOT, sharp_frame

pytestmark = pytest.mark.gpu

N_NXN = 64                                                             # NxN 8x8 CUs per set; the builder's other 8 tiles: four 2Nx2N 8x8 and four 16x16 CUs (the predicate is false)
OUTPUTS = ("d_sresults", "d_results", "d_cresults", "d_coef", "d_reco_y", "d_reco_c", "d_syntax_out", "d_dist", "d_bits", "d_cost", "d_ctx_out", "d_cu_ctx_out")
# (name, environment): the forms of the candidate chain, each with and without the switch
FORMS = [("side by side", {}), ("one after the other", {"HOP_WALK_CAND": "0"}), ("batch steps", {"HOP_WALK": "0"})]
SWITCH = "HOP_INTRA_FINAL_ALWAYS"


@pytest.fixture(scope="module")
def hp():
    spec = importlib.util.spec_from_file_location("hophip", os.path.join(ROOT, "hevc-hop_amd", "hophip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _zx(p): return 4 * sum(((p >> (2 * b)) & 1) << b for b in range(4))
def _zy(p): return 4 * sum(((p >> (2 * b + 1)) & 1) << b for b in range(4))
def _zidx(ux, uy): return sum((((ux >> b) & 1) << (2 * b)) | (((uy >> b) & 1) << (2 * b + 1)) for b in range(4))


def causal_avail(lg):
    """hop_intra_rqt_opt.avail of a CU of size 1 << lg with everything above and to the left of it coded: per node (341 entries: depth, then the node's position in z order)
    one bit per 4-sample unit -- below-left (bottom-most first) and left upwards, the corner, above, above-right -- set where the unit lies outside the CU above it or beside
    it, or inside the CU before the node in coding order.  What an encoder hands over; the builder's random tables may call samples of the CU available that are coded later,
    and then the side-by-side candidates (each started from the picture as it was) and the candidate-after-candidate forms read different samples."""
    cu = 1 << lg; first = (0, 1, 5, 21, 85)
    out = np.zeros(341, np.uint64)
    for d in range(lg - 1):
        log2 = lg - d; N = 1 << log2; U = N // 4
        for idx in range(4 ** d):
            part = idx << (2 * (log2 - 2)); bx, by = _zx(part), _zy(part)
            def ok(sx, sy):
                if sy < 0: return True
                if sx < 0: return sy < cu
                return sx < cu and sy < cu and _zidx(sx // 4, sy // 4) < part
            units = [(bx - 1, by + 4 * (2 * U - 1 - u)) for u in range(2 * U)] + [(bx - 1, by - 1)] + [(bx + 4 * j, by - 1) for j in range(2 * U)]
            out[first[d] + idx] = sum(1 << u for u, (sx, sy) in enumerate(units) if ok(sx, sy))
    return out


def build_set(hp, kind):
    """72 CUs in the tiles of tests/test_gpu_tq_intra.py's intra random-case builder (its pictures, coder states, QPs, lambdas, sign hiding / transform skip /
    TransformSkipFast / strong smoothing per CU): the first 64 as NxN 8x8 CUs, then four 2Nx2N 8x8 and four 16x16 CUs, availability as an encoder gives it.
    kind "noisy": the builder's content (a smooth field, coding noise around the CU, spikes).  kind "ties": original AND reconstruction from tests/degenerate.py, the upper
    tile rows the exactly 8-periodic picture, the lower ones flat -- candidates of exactly equal cost, where only the strict '<' of the decisions keeps the first."""
    from test_gpu_tq_intra import _irqt_random_cases
    bd = 8
    W, H, Y, R, jobs, syn, opts, cfgs, snaps, cus, avs = _irqt_random_cases(hp, hp.load(), bd)
    n = len(jobs); assert n == N_NXN + 8
    rng = np.random.default_rng(211)
    if kind == "ties":
        half = (H // 2) // 192 * 192
        Y = np.concatenate([dg.tile(W, half, 8, 8, bd)[0], dg.flat(W, H - half, "mid", bd)[0]]); R = Y.copy()
        C = [np.full((H // 2, W // 2), 128, np.int16) for _ in range(2)]; RC = [c.copy() for c in C]
    else:
        C = [np.clip(Y[::2, ::2] // 2 + 60 + k * 9, 0, 255).astype(np.int16) for k in range(2)]
        RC = [rng.integers(0, 256, (H // 2, W // 2)).astype(np.int16) for _ in range(2)]
    sj = np.zeros(n, hp.INTRA_SEARCH_JOB_DTYPE)
    sj["left_dir"] = rng.integers(0, 35, (n, 4)); sj["above_dir"] = rng.integers(0, 35, (n, 4)); sj["rough_flags"] = 1
    for i in range(n):
        lg, nxn = (3, 1) if i < N_NXN else (3, 0) if i < N_NXN + 4 else (4, 0)
        j = jobs[i]; s = syn[i]
        j["log2_cu"], j["log2_min_tu_in_cu"] = lg, 2
        if not nxn: j["sign_hide"], j["use_ts"] = 1, 1                  # (one class each)
        s["part_nxn"], s["is_min_cu"], s["tr_depth"], s["part"] = nxn, int(lg == 3), nxn, 0
        opts[i]["avail"] = causal_avail(lg)
        sj[i]["sqrt_lambda"] = float(np.sqrt(j["lambda_rd"])); sj[i]["num_full_rd"] = 8 if ((1 << lg) >> nxn) <= 8 else 3
    return dict(W=W, H=H, bd=bd, Y=Y, R=R, C=C, RC=RC, jobs=jobs, syn=syn, opts=opts, sj=sj, snaps=snaps, cus=cus)


def run_set(hp, S, monkeypatch):
    """the set through hop_intra_cu_device_classes in every form, with and without the switch: {(form, switch): {name: bytes}}"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    jobs, syn, opts, sj = S["jobs"], S["syn"], S["opts"], S["sj"]
    CLS = np.dtype([("n", "<i4"), ("part_nxn", "<i4"), ("num_full_rd", "<i4"), ("pad", "<i4"), ("cls", hp.RQT_JOB_DTYPE)] + [(k, "<u8") for k in
                   ("d_jobs", "d_syntax", "d_opts", "d_sjobs") + OUTPUTS])
    groups = {}
    for i in range(len(jobs)):
        j = jobs[i]; groups.setdefault((int(j["log2_cu"]), int(j["log2_min_tu_in_cu"]), int(j["sign_hide"]), int(j["use_ts"]), int(syn[i]["part_nxn"])), []).append(i)
    assert sum(len(v) for k, v in groups.items() if k[4]) == N_NXN and sum(1 for k in groups if not k[4]) == 2
    d_snap = up(S["snaps"]); d_cus = up(S["cus"])
    descs = np.zeros(len(groups), CLS); keep = []
    for gi, (key, idx) in enumerate(sorted(groups.items())):
        m = len(idx); cu = 1 << key[0]
        jj = jobs[idx].copy(); jj["ctx_index"] = idx
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        bufs = dict(d_jobs=up(jj), d_syntax=up(syn[idx]), d_opts=up(opts[idx]), d_sjobs=up(sj[idx]),
                    d_sresults=z(m * hp.INTRA_SEARCH_RESULT_DTYPE.itemsize), d_results=z(m * hp.RQT_RESULT_DTYPE.itemsize), d_cresults=z(m * 8), d_coef=z(m * cu * cu * 3 // 2 * 4),
                    d_reco_y=z(m * cu * cu * 2), d_reco_c=z(m * cu * cu // 2 * 2), d_syntax_out=z(m * hp.INTRA_CU_SYNTAX_DTYPE.itemsize), d_dist=z(m * 4), d_bits=z(m * 4),
                    d_cost=z(m * 8), d_ctx_out=z(m * hp.CABAC_CTX_BYTES), d_cu_ctx_out=z(m * hp.CABAC_CU_CTX_BYTES))
        d = descs[gi]; d["n"], d["part_nxn"], d["num_full_rd"], d["cls"] = m, key[4], int(sj[idx[0]]["num_full_rd"]), jj[0]
        for name, t in bufs.items(): d[name] = t.data_ptr()
        keep.append(bufs)
    out = {}
    for form, env in FORMS:
        for k in ("HOP_WALK_CAND", "HOP_WALK"): monkeypatch.delenv(k, raising=False)
        for k, v in env.items(): monkeypatch.setenv(k, v)
        ctx = hp.Context(S["W"], S["H"], S["bd"])                           # (HOP_WALK is read when a context is created, the other two per call)
        ctx.upload_orig(S["Y"], S["C"][0], S["C"][1])
        ctx.L.hop_intra_cu_device_classes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        for switch in (0, 1):
            if switch: monkeypatch.setenv(SWITCH, "1")
            else: monkeypatch.delenv(SWITCH, raising=False)
            ctx.plane_upload("recon", 0, S["R"])
            for k in range(2): ctx.plane_upload("recon", 1 + k, S["RC"][k])
            for b in keep:
                for name in OUTPUTS: b[name].zero_()
            ctx._chk(ctx.L.hop_intra_cu_device_classes(ctx.h, len(descs), descs.ctypes.data, d_snap.data_ptr(), d_cus.data_ptr()), "hop_intra_cu_device_classes")
            ctx.sync()
            got = {name: b"".join(b[name].cpu().numpy().tobytes() for b in keep) for name in OUTPUTS}
            for k in range(3): got["recon%d" % k] = ctx.recon_download(k).tobytes()
            out[(form, switch)] = got
        ctx.close()
    monkeypatch.delenv(SWITCH, raising=False)
    return out, keep, sorted(groups)


@pytest.mark.parametrize("kind", ["noisy", "ties"])
def test_final_pass_switch_changes_no_byte_of_the_kernel_entry(hp, kind, monkeypatch):
    """64 NxN 8x8 CUs (the final pass of every PU is a repeat and is left out) beside one class of 2Nx2N 8x8 and one of 16x16 CUs (it is not: the switch must change
    nothing there either) through hop_intra_cu_device_classes: search results, transform-tree arrays, chroma results, levels, reconstructed blocks, syntax elements,
    distortion / bits / cost, the coder states and the context's three reconstruction planes are the same bytes in all six runs."""
    S = build_set(hp, kind)
    out, keep, keys = run_set(hp, S, monkeypatch)
    ref_key = (FORMS[0][0], 1)                                            # the old behaviour in the default form
    ref = out[ref_key]
    for key, got in out.items():
        for name in ref:
            assert got[name] == ref[name], (kind, key, "differs from", ref_key, "in", name)
    # the runs did something: costs, and NxN CUs with four decided directions
    cost = np.frombuffer(ref["d_cost"], np.float64); assert (cost > 0).all()
    sres = np.frombuffer(ref["d_sresults"], hp.INTRA_SEARCH_RESULT_DTYPE)
    assert len(sres) == N_NXN + 8 and (sres["n_cand"][:, 0] >= 1).all()
    nxn = np.concatenate([np.full(int(b["d_dist"].numel()) // 4, k[4]) for b, k in zip(keep, keys)]).astype(bool)
    assert int(nxn.sum()) == N_NXN and (sres["n_cand"][nxn] >= 1).all()
    if kind == "noisy":
        assert np.frombuffer(ref["recon0"], np.int16).tobytes() != np.ascontiguousarray(S["R"], np.int16).tobytes()


def test_final_pass_switch_changes_no_byte_of_an_encoded_picture(hp, monkeypatch):
    """one 128x64 picture of sharp content (the CPU spine over the restatement codes some eighty of its 8x8 CUs as intra NxN), --MIsize=15, QP 32, through hop_encode_frame
    as a lag-2 wavefront, with and without the switch: costs, bits, distortions, partition records and the reconstruction are the same bytes, and NxN CUs were chosen"""
    W, H = 128, 64
    Y, Cb, Cr = sharp_frame(W, H, 4)
    runs = []
    for switch in (0, 1):
        if switch: monkeypatch.setenv(SWITCH, "1")
        else: monkeypatch.delenv(SWITCH, raising=False)
        ctx = hp.Context(W, H, slots=16)
        ctx.upload_orig(Y, Cb, Cr)
        cost, bits, dist, parts, nc = ctx.encode_frame(32, 15, wpp=1, wavefront_lag=2)
        runs.append((cost.tobytes(), bits.tobytes(), dist.tobytes(), parts.tobytes(), nc, [ctx.recon_download(k).tobytes() for k in range(3)]))
        ctx.close()
        nxn = (parts["pred_mode"] == 1) & (parts["part_size"] == 3) & (parts["depth"] == 3)      # MODE_INTRA, SIZE_NxN, per 4x4 partition: four records per CU
        assert int(nxn.sum()) >= 4, "no intra NxN CU in the partition records: the picture does not exercise the path"
    monkeypatch.delenv(SWITCH, raising=False)
    for k, name in enumerate(("cost", "bits", "dist", "parts", "candidates", "recon")):
        assert runs[0][k] == runs[1][k], name
