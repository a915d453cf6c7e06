"""GPU: the one-lane coders' bin table in LDS and the closed forms of the small index tables (csrc/hop_cabac_tab.h) against the 64-lanes-per-wave coder.

Wherever one lane codes a CU or a transform unit (the candidate walks, the fused leaf kernels, the workgroup-per-CU launches of the batch steps) a context-coded bin reads
the workgroup's packed table in LDS; the batch steps of a class of ONE candidate (HOP_WALK=0, n = 1) run the 64-lane form, which reads the __constant__ tables as before.
So every candidate of a class of five runs in the three forms of the chain (side by side, HOP_WALK_CAND=0, HOP_WALK=0) and once more ALONE through the batch steps; every
output of the four, and the candidate's reconstruction planes, must be the same bytes.

Cases and runs are those of tests/test_gpu_walk_codegen.py (its case builder, its runner, its nine classes); what this file changes is the content, so that every bin-coding
path is reached: a uniform-random 8-bit original at QP 4 and at QP 22 (large levels: Rice parameter 4, the escape prefix loop, more than eight levels above 1 in a group,
last positions far out, transform skip) beside lenslet content at QP 32 (the flagship's).  test_content_reaches_every_bin_path asserts from the returned levels that it does.

Time: 27 cases of 8 runs each (a context per run); the budget for the file is 20 s on one MI355X."""
import numpy as np
import pytest

import test_gpu_walk_codegen as walk
from test_gpu_walk_codegen import CLASSES, FORMS, H, W, X0, Y0, _ident, hp  # noqa: F401  (hp: the module's fixture)
from hoputil import lenslet

pytestmark = pytest.mark.gpu

N = 5
CONTENTS = [("random-qp4", 4), ("random-qp22", 22), ("lenslet-qp32", 32)]
_levels = {}                                                           # (class, content) -> what the staged chain returned, for the content test


def _patched_case(hp, cls, content, qp):
    """the walk test's noisy case of five candidates with this file's original (and, for inter lenslet content, a prediction one micro-image away) and QP"""
    side, lg, nxn = cls
    C = dict(walk._case(hp, side, lg, nxn, N, "noisy"))
    cu = 1 << lg
    rng = np.random.default_rng(77 * lg + 7 * nxn + qp + (side == "intra"))
    org = [[a.copy() for a in C["org"][k]] for k in range(3)]; pred = [[a.copy() for a in C["pred"][k]] for k in range(3)]
    jobs = C["jobs"].copy()
    for t in range(N):
        if content.startswith("random"):
            blk = [rng.integers(0, 256, (64, 64)).astype(np.int16), rng.integers(0, 256, (32, 32)).astype(np.int16), rng.integers(0, 256, (32, 32)).astype(np.int16)]
            pblk = None
        else:
            P = lenslet(W + 16, H, 15, 300 + 10 * lg + t)
            blk = [P[0][Y0:Y0 + 64, X0:X0 + 64], P[1][Y0 // 2:Y0 // 2 + 32, X0 // 2:X0 // 2 + 32], P[2][Y0 // 2:Y0 // 2 + 32, X0 // 2:X0 // 2 + 32]]
            pblk = [P[0][Y0:Y0 + 64, X0 - 15:X0 + 49], P[1][Y0 // 2:Y0 // 2 + 32, X0 // 2 - 7:X0 // 2 + 25], P[2][Y0 // 2:Y0 // 2 + 32, X0 // 2 - 7:X0 // 2 + 25]]
        for k in range(3):
            s = 1 if k else 0; c = cu >> s
            org[k][t][Y0 >> s:(Y0 >> s) + c, X0 >> s:(X0 >> s) + c] = blk[k][:c, :c]
            if side == "inter" and pblk is not None: pred[k][t][Y0 >> s:(Y0 >> s) + c, X0 >> s:(X0 >> s) + c] = pblk[k][:c, :c]
        lam = 0.57 * 2.0 ** ((qp - 12) / 3.0); w = float(jobs[t]["dist_weight"][0])
        jobs[t]["qp_scaled"] = (qp, qp - 1, qp - 2); jobs[t]["lambda_rd"] = lam; jobs[t]["lambda_rdoq"] = (lam, lam / w, lam / w)
    C.update(org=org, pred=pred, jobs=jobs)
    if side == "intra":
        sj = C["sj"].copy(); sj["sqrt_lambda"] = np.sqrt(jobs["lambda_rd"]); C["sj"] = sj
    return C


def _single(C, t):
    """candidate t of the case alone (its picture stays where it is in the stack)"""
    S = dict(C); S["n"] = 1
    for name in ("jobs", "snaps", "cus", "syn", "opts", "sj"):
        if name in C: S[name] = C[name][t:t + 1].copy()
    S["jobs"]["ctx_index"] = 0
    return S


def _picture_rows(hp, plane_bytes, comp, t):
    ctx = hp.Context(W, H, pictures=walk.PICS); pitch = ctx.pitch; ctx.close()
    s = 1 if comp else 0
    a = np.frombuffer(plane_bytes, np.int16).reshape(-1, W >> s)
    return a[(t * pitch) >> s:((t * pitch) >> s) + (H >> s)].tobytes()


@pytest.mark.parametrize("content,qp", CONTENTS, ids=[c for c, _ in CONTENTS])
@pytest.mark.parametrize("cls", CLASSES, ids=_ident)
def test_one_lane_coders_give_the_64_lane_coder_byte_for_byte(hp, cls, content, qp):
    _compare(hp, cls, content, qp)


def _compare(hp, cls, content, qp):
    """the comparisons of one (class, content), once per session; leaves the staged chain's levels in _levels"""
    if (cls, content) in _levels: return
    mine = []
    def seed(n, name, case):
        walk._runs[("case", cls, n, name)] = case; mine.append(name)
    try:
        C = _patched_case(hp, cls, content, qp)
        seed(N, content, C)
        ref = walk._run(hp, cls, N, content, FORMS[2][1])                   # the batch steps over five candidates (a workgroup per CU: the one-lane form too)
        for form, env in FORMS[:2]:
            got = walk._run(hp, cls, N, content, env)
            for name in ref:
                assert got[name] == ref[name], (_ident(cls), content, form, "differs from the batch steps in", name)
        for t in range(N):                                                  # each candidate alone: one lane of a wave of 64, the __constant__ tables
            name1 = "%s#%d" % (content, t)
            seed(1, name1, _single(C, t))
            one = walk._run(hp, cls, 1, name1, FORMS[2][1])
            for name in ref:
                if name.startswith("recon"):
                    k = int(name[5:])
                    assert _picture_rows(hp, one[name], k, t) == _picture_rows(hp, ref[name], k, t), (_ident(cls), content, "candidate", t, "alone differs in", name)
                else:
                    sz = len(ref[name]) // N
                    assert one[name] == ref[name][t * sz:(t + 1) * sz], (_ident(cls), content, "candidate", t, "alone differs in", name)
        _levels[(cls, content)] = dict(coef=np.frombuffer(ref["d_coef"], np.int32).copy(), res=np.frombuffer(ref["d_results"], hp.RQT_RESULT_DTYPE).copy(),
                                       syn=np.frombuffer(ref["d_syntax_out"], hp.INTRA_CU_SYNTAX_DTYPE).copy() if cls[0] == "intra" else None)
    finally:
        for key in [k for k in walk._runs if (k[3] if k[0] == "case" else k[2]) in mine]:      # (the runner memoises cases and runs: this file's go again)
            del walk._runs[key]


def _diag(n):
    """scan position of (y, x) in the up-right diagonal scan of an n x n grid"""
    idx = np.zeros((n, n), np.int32); p = 0
    for s in range(2 * n - 1):
        for y in range(min(s, n - 1), -1, -1):
            x = s - y
            if x < n: idx[y, x] = p; p += 1
    return idx


def _luma_units(lg, r, coef_cu):
    """the luma transform units of one CU: (log2, transform-skip flag, levels as a raster block), from the tree in tr_idx and the z-ordered level layout"""
    parts = 1 << (2 * (lg - 2)); p = 0
    while p < parts:
        log2 = lg - int(r["tr_idx"][p]); n_p = 1 << (2 * (log2 - 2)); side = 1 << log2
        yield log2, int(r["tskip"][0][p]), coef_cu[16 * p:16 * (p + n_p)].reshape(side, side)
        p += n_p


def test_content_reaches_every_bin_path(hp):
    """from the levels the staged chain returned: the escape prefix loop, more than eight levels above 1 in a group, the last position's suffix bins, the three scan
    orders of intra 8x8, a 4x4 unit with transform skip"""
    for cls in CLASSES:
        for content, qp in CONTENTS: _compare(hp, cls, content, qp)            # (memoised: run here only where this test is selected alone)
    big = crowded = ts4 = False
    far = {4: False, 5: False}
    scans = set()
    for (cls, content), got in _levels.items():
        side, lg, nxn = cls; cu2 = 1 << (2 * lg)
        for t in range(N):
            cu_coef = got["coef"][t * cu2 * 3 // 2:(t + 1) * cu2 * 3 // 2]
            big |= bool((np.abs(cu_coef) > (3 << 4)).any())
            for log2, ts, blk in _luma_units(lg, got["res"][t], cu_coef[:cu2]):
                g = 1 << (log2 - 2)
                groups = np.abs(blk).reshape(g, 4, g, 4).transpose(0, 2, 1, 3).reshape(g, g, 16)
                crowded |= bool(((groups > 1).sum(axis=2) > 8).any())
                ts4 |= bool(log2 == 2 and ts and blk.any())
                if log2 >= 4 and lg in far and blk.any():                  # (16x16 and 32x32 units are scanned diagonally whatever the direction)
                    pos = 16 * _diag(g)[:, None, :, None] + _diag(4)[None, :, None, :]
                    pos = np.where(blk.reshape(g, 4, g, 4) != 0, pos, -1)
                    ly, lx = divmod(int(np.argmax(pos.reshape(1 << log2, 1 << log2))), 1 << log2)
                    far[lg] |= max(ly, lx) >= 8
            if side == "intra" and lg == 3:
                for d in got["syn"][t]["luma_dir"][:4 if nxn else 1]:
                    scans.add(2 if 6 <= d <= 14 else 1 if 22 <= d <= 30 else 0)
    assert big, "no |level| above 3 << 4: Rice parameter 4 and the escape prefix loop are not reached"
    assert crowded, "no coefficient group with more than eight levels above 1"
    assert far[4] and far[5], ("no last position with a coordinate of 8 or more in the 16x16 / 32x32 classes", far)
    assert scans == {0, 1, 2}, ("the intra 8x8 classes do not choose directions of all three scan orders", scans)
    assert ts4, "no 4x4 unit chosen with transform skip"
