"""A plain reference decoder for hop_decode_frame's input: Python over the CPU oracle's primitives (oracle/libhop_oracle.so), host only, written to be read.

ref_decode follows TDecCu::xDecompressCU as include/hophip.h describes it: CTUs in raster order, CUs in z-order, an intra CU's luma TUs and then its chroma TUs each
predicted from the reconstruction so far, an SS/GT CU's PUs predicted from the SS reference and the residual quadtree added, every CU of a non-plain picture committed
to the SS reference.  It shares no code with the library (it neither imports hophip nor loads libhophip.so), and it states intra availability differently: not by
z-order comparisons but by a per-plane map of the samples reconstructed so far -- a neighbour unit is available when it lies inside the picture and is set in the map.
tests/test_refdecode_cpu.py pins it to the CPU spine's reconstruction (itself pinned to the reference encoder) before anything is measured against it."""
import ctypes

import numpy as np

from hoputil import Planes, oracle

PART_FIELDS = ("depth", "pred_mode", "part_size", "skip", "merge_flag", "gt_flag", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "mv", "gt")
DM_CHROMA = 36


def zpos(z):
    """4x4-unit coordinates of z-order index z inside a CTU"""
    x = y = 0
    for b in range(4):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def zidx(x4, y4):
    z = 0
    for b in range(4):
        z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1))
    return z


def pu_rect(ps, S, pu):
    """TComDataCU::getPartIndexAndSize: offset and size of PU `pu` of part size `ps` in a CU of S samples"""
    q, h = S >> 2, S >> 1
    if ps == 0: return 0, 0, S, S
    if ps == 1: return 0, h * pu, S, h
    if ps == 2: return h * pu, 0, h, S
    if ps == 3: return h * (pu & 1), h * (pu >> 1), h, h
    if ps == 4: return (0, 0, S, q) if pu == 0 else (0, q, S, q + h)
    if ps == 5: return (0, 0, S, q + h) if pu == 0 else (0, q + h, S, q)
    if ps == 6: return (0, 0, q, S) if pu == 0 else (q, 0, q + h, S)
    if ps == 7: return (0, 0, q + h, S) if pu == 0 else (q + h, 0, q, S)
    raise ValueError("part size %d" % ps)


def num_pus(ps):
    return 1 if ps == 0 else 4 if ps == 3 else 2


def clip_mv(W, H, cx, cy, mvx, mvy):
    """TComDataCU::clipMv at the CU's position: the displaced CU stays within 8 samples of the picture plus one CTU to the left / above"""
    hmax, hmin = (W + 8 - cx - 1) * 4, (-64 - 8 - cx + 1) * 4
    vmax, vmin = (H + 8 - cy - 1) * 4, (-64 - 8 - cy + 1) * 4
    return min(hmax, max(hmin, mvx)), min(vmax, max(vmin, mvy))


def chroma_qp_scaled(qp, offset, bit_depth):
    """TComTrQuant::setQPforQuant for a chroma plane: qPi = Clip3(-QpBdOffset, 57, qp + offset); negative: unchanged; else through the standard's table (identity below
    30, the list for 30..43, qPi - 6 above); plus QpBdOffset"""
    bdo = 6 * (bit_depth - 8)
    qpi = min(57, max(-bdo, qp + offset))
    if qpi < 0:
        return qpi + bdo
    if qpi < 30:
        qpc = qpi
    elif qpi <= 43:
        qpc = (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)[qpi - 30]
    else:
        qpc = qpi - 6
    return qpc + bdo


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class _Decoder:
    def __init__(self, W, H, qp, cb_off, cr_off, bd, plain):
        self.O = oracle()
        self.W, self.H, self.bd, self.plain = W, H, bd, plain
        self.dims = [(W, H), (W >> 1, H >> 1), (W >> 1, H >> 1)]
        self.rec = [np.zeros((h, w), np.int16) for w, h in self.dims]
        self.done = [np.zeros((h, w), bool) for w, h in self.dims]         # samples reconstructed so far, per plane
        self.qp = [qp + 6 * (bd - 8), chroma_qp_scaled(qp, cb_off, bd), chroma_qp_scaled(qp, cr_off, bd)]
        self.pl = None
        if not plain:
            self.pl = Planes(W, H)
            self.O.hop_o_ssref_reset(_p(self.pl.bufY), _p(self.pl.bufCb), _p(self.pl.bufCr), W, H)

    # ---- intra prediction of one block of one plane at plane coordinates (x, y) ----
    def flags(self, comp, x, y, N, unit):
        """availability per unit in the order of the reference's bNeighborFlags: below-left (bottom-most first) and left upwards, the corner, above and above-right"""
        pw, ph = self.dims[comp]
        done = self.done[comp]
        U = N // unit

        def avail(sx, sy):
            return 1 if 0 <= sx < pw and 0 <= sy < ph and done[sy, sx] else 0
        f = np.zeros(4 * U + 1, np.uint8)
        for u in range(2 * U):
            f[u] = avail(x - 1, y + unit * (2 * U - 1 - u))
        f[2 * U] = avail(x - 1, y - 1)
        for j in range(2 * U):
            f[2 * U + 1 + j] = avail(x + unit * j, y - 1)
        return f

    def intra_pred(self, comp, x, y, N, mode):
        O, rec = self.O, self.rec[comp]
        L = (ctypes.c_int * (4 * N + 1))()
        pred = np.zeros((N, N), np.int16)
        if comp == 0:
            f = self.flags(0, x, y, N, 4)
            O.hop_o_intra_fill_refs(_p(rec), rec.shape[1], x, y, N, _p(f), self.bd, L)
            F = (ctypes.c_int * (4 * N + 1))()
            O.hop_o_intra_smooth(L, N, self.bd, 1, F)                      # strong_intra_smoothing on in both configurations
            O.hop_o_intra_pred(L, F, N, mode, self.bd, _p(pred))
        else:
            f = self.flags(comp, x, y, N, 2)
            O.hop_o_intra_fill_refs_u(_p(rec), rec.shape[1], x, y, N, 2, _p(f), self.bd, L)
            O.hop_o_intra_pred_chroma(L, N, mode, self.bd, _p(pred))
        return pred

    # ---- one TU: clip(prediction + inverse residual) into the plane, or the prediction for cbf 0 ----
    def tu(self, comp, x, y, N, pred, cbf, tskip, dst, lv):
        O = self.O
        out = pred
        if cbf:
            level = np.ascontiguousarray(lv[:N * N], np.int32)
            coef = np.zeros(N * N, np.int32)
            resi = np.zeros((N, N), np.int16)
            O.hop_o_dequant_flat(self.bd, self.qp[comp], _p(level), _p(coef), N)
            if tskip:
                O.hop_o_inv_transform_skip(self.bd, _p(coef), _p(resi), N)
            else:
                c16 = coef.astype(np.int16)
                O.hop_o_inv_transform(self.bd, _p(c16), _p(resi), N, 1 if dst else 0)
            out = np.clip(pred.astype(np.int32) + resi, 0, (1 << self.bd) - 1).astype(np.int16)
        self.rec[comp][y:y + N, x:x + N] = out
        self.done[comp][y:y + N, x:x + N] = True

    def intra_cu(self, P, LV, z, ox, oy, log2cu):
        """xReconIntraQT: ox, oy = the CTU's position"""
        np_ = 1 << (2 * (log2cu - 2))
        u = 0
        while u < np_:
            q = P[z + u]
            l2 = log2cu - int(q["tr_idx"]); N = 1 << l2
            x4, y4 = zpos(z + u); x, y = ox + 4 * x4, oy + 4 * y4
            pred = self.intra_pred(0, x, y, N, int(q["luma_dir"]))
            self.tu(0, x, y, N, pred, (int(q["cbf"][0]) >> int(q["tr_idx"])) & 1, q["tskip"][0] != 0, N == 4, LV[16 * (z + u):])
            u += 1 << (2 * (l2 - 2))
        mode = int(P[z]["chroma_dir"])
        if mode == DM_CHROMA:
            mode = int(P[z]["luma_dir"])                                   # the luma direction of the CU's first unit
        u = 0
        while u < np_:
            q = P[z + u]
            l2 = log2cu - int(q["tr_idx"])
            tn, Nc, bit = 1 << (2 * (l2 - 2)), 1 << (l2 - 1), int(q["tr_idx"])
            if l2 == 2:                                                    # the 4x4 chroma block of four 4x4 luma TUs: the parent 8x8 node's, done with the first
                tn, Nc, bit = 4, 4, int(q["tr_idx"]) - 1
            x4, y4 = zpos(z + u); x, y = (ox + 4 * x4) >> 1, (oy + 4 * y4) >> 1
            for comp in (1, 2):
                pred = self.intra_pred(comp, x, y, Nc, mode)
                self.tu(comp, x, y, Nc, pred, (int(q["cbf"][comp]) >> bit) & 1, q["tskip"][comp] != 0, False, LV[(4096 if comp == 1 else 5120) + 4 * (z + u):])
            u += tn

    def inter_cu(self, P, LV, z, ox, oy, log2cu):
        """xReconInter: every PU from the SS reference, then the residual quadtree"""
        O, pl = self.O, self.pl
        S = 1 << log2cu
        x4, y4 = zpos(z); cx, cy = ox + 4 * x4, oy + 4 * y4
        pred = [np.zeros((S, S), np.int16), np.zeros((S >> 1, S >> 1), np.int16), np.zeros((S >> 1, S >> 1), np.int16)]
        ps = int(P[z]["part_size"])
        for pu in range(num_pus(ps)):
            px, py, w, h = pu_rect(ps, S, pu)
            p = P[zidx(((cx & 63) + px) >> 2, ((cy & 63) + py) >> 2)]
            mx, my = clip_mv(self.W, self.H, cx, cy, int(p["mv"][0]), int(p["mv"][1]))
            use_gt = 1 if (not p["merge_flag"] and p["gt_flag"]) else 0
            out = [np.zeros((h, w), np.int16), np.zeros((h >> 1, w >> 1), np.int16), np.zeros((h >> 1, w >> 1), np.int16)]
            O.hop_o_pred_inter(pl.ptr00(0), pl.sy, pl.ptr00(1), pl.ptr00(2), pl.sc, cx + px, cy + py, w, h, mx, my, use_gt, (ctypes.c_int * 8)(*[int(v) for v in p["gt"]]),
                               8, 8, _p(out[0]), _p(out[1]), _p(out[2]))
            pred[0][py:py + h, px:px + w] = out[0]
            for c in (1, 2):
                pred[c][py >> 1:(py + h) >> 1, px >> 1:(px + w) >> 1] = out[c]
        np_ = 1 << (2 * (log2cu - 2))
        u = 0
        while u < np_:
            q = P[z + u]
            tr = int(q["tr_idx"]); l2 = log2cu - tr; N = 1 << l2
            x4, y4 = zpos(z + u); x, y = ox + 4 * x4, oy + 4 * y4
            self.tu(0, x, y, N, pred[0][y - cy:y - cy + N, x - cx:x - cx + N], (int(q["cbf"][0]) >> tr) & 1, q["tskip"][0] != 0, False, LV[16 * (z + u):])
            if l2 > 2 or (z + u) % 4 == 0:
                Nc, bit = (N >> 1, tr) if l2 > 2 else (4, tr - 1)
                xc, yc = x >> 1, y >> 1
                for comp in (1, 2):
                    pc = pred[comp][yc - (cy >> 1):yc - (cy >> 1) + Nc, xc - (cx >> 1):xc - (cx >> 1) + Nc]
                    self.tu(comp, xc, yc, Nc, pc, (int(q["cbf"][comp]) >> bit) & 1, q["tskip"][comp] != 0, False, LV[(4096 if comp == 1 else 5120) + 4 * (z + u):])
            u += 1 << (2 * (l2 - 2))

    def commit(self, cx, cy, S):
        """xFindSSRef2Copy: the CU into the SS reference, all borders re-extended"""
        pl = self.pl
        b = [np.ascontiguousarray(self.rec[0][cy:cy + S, cx:cx + S])] + [np.ascontiguousarray(self.rec[c][cy >> 1:(cy + S) >> 1, cx >> 1:(cx + S) >> 1]) for c in (1, 2)]
        self.O.hop_o_ssref_commit_cu(pl.ptr00(0), pl.ptr00(1), pl.ptr00(2), self.W, self.H, cx, cy, S, _p(b[0]), _p(b[1]), _p(b[2]))


def ref_decode(W, H, parts, levels, qp, cb_off, cr_off, bit_depth, plain_intra):
    """parts: (n_ctu, 256) structured array with the fields of hop_cu_part; levels: (n_ctu, 6144) int32.  Returns (rec[3], ssref[3] or None): the reconstruction planes and,
    for a picture of the HOP configuration, the three padded SS-reference planes (margins 80 / 40)."""
    assert plain_intra or bit_depth == 8
    d = _Decoder(W, H, qp, cb_off, cr_off, bit_depth, plain_intra)
    wctu = (W + 63) // 64
    levels = np.asarray(levels).reshape(-1, 6144)
    for a in range(parts.shape[0]):
        P, LV = parts[a], levels[a]
        ox, oy = (a % wctu) * 64, (a // wctu) * 64
        z = 0
        while z < 256:
            mode = int(P[z]["pred_mode"])
            if mode not in (0, 1):                                         # outside the picture
                z += 1
                continue
            log2cu = 6 - int(P[z]["depth"])
            if mode == 1:
                d.intra_cu(P, LV, z, ox, oy, log2cu)
            else:
                assert not plain_intra
                d.inter_cu(P, LV, z, ox, oy, log2cu)
            if not plain_intra:
                x4, y4 = zpos(z)
                d.commit(ox + 4 * x4, oy + 4 * y4, 1 << log2cu)
            z += 1 << (2 * (log2cu - 2))
    assert all(m.all() for m in d.done)
    ss = None if plain_intra else [np.array(b) for b in (d.pl.bufY, d.pl.bufCb, d.pl.bufCr)]
    return d.rec, ss
