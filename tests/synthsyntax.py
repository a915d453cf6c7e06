"""A deterministic generator of valid syntax for hop_decode_frame: partition data and levels no encoder chose.

make_case(name) -> dict(W, H, bd, plain, qp, cb_off, cr_off, parts, levels, coverage): seeded, no files.  The pictures are laid out from lists of CUs that must
occur (every luma direction at every TU size, every part size at every CU size, ...), packed bottom-up into quadtrees and dealt to the whole CTUs in shuffled order;
the partial CTUs at the right and bottom border take 8x8 CUs.  Vectors and GT corners are bounded by this file's own arithmetic (fits()): block, interpolation taps
and the GT patch stay inside the padded plane (margin 80 luma, 40 chroma) and its 64 guard rows above and below; the library's own checks are not consulted.
coverage(case) reads back what a finished case contains from its parts alone; fill_levels adds the (shape, magnitude) pairs it made.

The pictures are larger than a first count suggests: 35 directions on 32x32 TUs need 35 CUs of 32x32, eight part sizes on 64x64 CUs eight whole CTUs."""
import functools

import numpy as np

PART_DT = np.dtype([("depth", "u1"), ("pred_mode", "u1"), ("part_size", "u1"), ("skip", "u1"), ("merge_flag", "u1"), ("merge_idx", "u1"), ("gt_flag", "u1"), ("inter_dir", "u1"),
                    ("ref_idx", "i1"), ("mvp_idx", "i1"), ("mvp_num", "i1"), ("luma_dir", "u1"), ("chroma_dir", "u1"), ("tr_idx", "u1"), ("cbf", "u1", 3), ("tskip", "u1", 3),
                    ("mv", "<i2", 2), ("mvd", "<i2", 2), ("gt", "<i2", 8)])                  # hop_cu_part (include/hophip.h)
MARGIN_Y, MARGIN_C, GUARD = 80, 40, 64
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)
CHROMA_DIRS = (0, 1, 10, 26, 34, 36, 2, 18, 7, 30)
SHAPES = ("dc", "last", "sparse", "dense")
MAGS = ("small", "mid", "large")
INTER_PART_SIZES = (0, 1, 2, 4, 5, 6, 7)      # NxN (3) is no part size of an SS/GT CU: the syntax has it at the smallest CU size only, and not for 8x8
MV_KINDS = ("decoded", "future", "own_cu", "margin", "clip")

# name -> (syntax, bit depth, plain_intra, qp, cb offset, cr offset)
CASES = {
    "intra_all":          ("intra_all", 8, 0, 22, 5, -3),
    "intra_all_10":       ("intra_all", 10, 1, 22, 0, 0),
    "intra_all_10_qpm12": ("intra_all", 10, 1, -12, -12, 12),
    "intra_all_10_qp51":  ("intra_all", 10, 1, 51, -12, 12),
    "inter_all":          ("inter_all", 8, 0, 32, 0, 0),
    "inter_all_qp51":     ("inter_all", 8, 0, 51, 5, -3),
    "mixed_local":        ("mixed_local", 8, 0, 0, -12, 12),
}
SIZES = {"intra_all": (392, 200), "inter_all": (392, 200), "mixed_local": (256, 192)}


def zpos(z):
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
    q, h = S >> 2, S >> 1
    return {0: [(0, 0, S, S)], 1: [(0, 0, S, h), (0, h, S, h)], 2: [(0, 0, h, S), (h, 0, h, S)], 3: [(0, 0, h, h), (h, 0, h, h), (0, h, h, h), (h, h, h, h)],
            4: [(0, 0, S, q), (0, q, S, q + h)], 5: [(0, 0, S, q + h), (0, q + h, S, q)], 6: [(0, 0, q, S), (q, 0, q + h, S)], 7: [(0, 0, q + h, S), (q + h, 0, q, S)]}[ps][pu]


def num_pus(ps):
    return 1 if ps == 0 else 4 if ps == 3 else 2


def clip_mv(W, H, cx, cy, mvx, mvy):
    return (min((W + 8 - cx - 1) * 4, max((-64 - 8 - cx + 1) * 4, mvx)), min((H + 8 - cy - 1) * 4, max((-64 - 8 - cy + 1) * 4, mvy)))


def fits(W, H, px, py, w, h, mvx, mvy, gt):
    """block, taps (counted whether or not the phase needs them) and, with GT, the doubled patch around the block, inside the padded planes and their guard rows"""
    for sh, m, tl, tr in ((0, MARGIN_Y, 3, 4), (1, MARGIN_C, 1, 2)):
        bx, by, bw, bh, pw, ph = px >> sh, py >> sh, w >> sh, h >> sh, W >> sh, H >> sh
        ix, iy = mvx >> (2 + sh), mvy >> (2 + sh)
        ex, ey = (bw // 2, bh // 2) if gt else (0, 0)
        if bx + ix - ex - tl < -m or bx + ix + bw - 1 + ex + tr >= pw + m: return False
        if by + iy - ey - tl < -m - GUARD or by + iy + bh - 1 + ey + tr >= ph + m + GUARD: return False
    return True


def level_bound(bd, qp_scaled, N):
    """the largest |level| the reference's own Int arithmetic is defined for (TComTrQuant::xDeQuant, flat): |v| * (invQuantScale[rem] << per) + add < 2^31, within the
    16-bit clip of the level (fill_levels caps at 32767 / -32768)"""
    log2n = {4: 2, 8: 3, 16: 4, 32: 5}[N]
    shift = 20 - 14 - (15 - bd - log2n)
    add = 1 << (shift - 1)
    scale = INV_QUANT_SCALES[qp_scaled % 6] << (qp_scaled // 6)
    return ((1 << 31) - 1 - add) // scale


def chroma_qp_scaled(qp, offset, bd):
    bdo = 6 * (bd - 8)
    qpi = min(57, max(-bdo, qp + offset))
    if qpi < 0: return qpi + bdo
    return (qpi if qpi < 30 else (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)[qpi - 30] if qpi <= 43 else qpi - 6) + bdo


# ---- the TUs of a CU, as the decoder walks them: (component, first unit, size in the plane's samples, cbf bit, units of the TU) ----
def cu_tus(P, z, log2cu):
    np_ = 1 << (2 * (log2cu - 2))
    out = []
    u = 0
    while u < np_:
        t = int(P[z + u]["tr_idx"]); l2 = log2cu - t; tn = 1 << (2 * (l2 - 2))
        out.append((0, z + u, 1 << l2, t, tn))
        if l2 > 2:
            out += [(c, z + u, 1 << (l2 - 1), t, tn) for c in (1, 2)]
        elif (z + u) % 4 == 0:
            out += [(c, z + u, 4, t - 1, 4) for c in (1, 2)]
        u += tn
    return out


def cus(parts):
    """(ctu, z, log2cu) of every CU"""
    for a in range(parts.shape[0]):
        z = 0
        while z < 256:
            if parts[a]["pred_mode"][z] > 1:
                z += 1
                continue
            l2 = 6 - int(parts[a]["depth"][z])
            yield a, z, l2
            z += 1 << (2 * (l2 - 2))


class _Builder:
    def __init__(self, W, H, seed):
        self.W, self.H = W, H
        self.wctu, self.hctu = (W + 63) // 64, (H + 63) // 64
        self.rng = np.random.RandomState(seed)
        self.parts = np.zeros((self.wctu * self.hctu, 256), PART_DT)
        self.parts["pred_mode"] = 15; self.parts["part_size"] = 15
        self.n_pu = 0          # cycles vector kinds, phases, margin sides
        self.n_tu = 0          # cycles the cbf combinations
        self.n_cdir = 0

    # -- transform tree: tr_idx per unit of a CU.  spec: an int (uniform) or "mix" (random splits) --
    def tr_units(self, log2cu, spec, nxn=False):
        np_ = 1 << (2 * (log2cu - 2))
        if spec != "mix":
            return np.full(np_, spec, np.uint8)
        out = np.zeros(np_, np.uint8)

        def rec(u0, d):
            l2 = log2cu - d
            must = l2 > 5 or (nxn and d == 0)
            if must or (l2 > 2 and d < 3 and self.rng.rand() < 0.5):
                n = np_ >> (2 * (d + 1))
                for k in range(4): rec(u0 + k * n, d + 1)
            else:
                out[u0:u0 + (np_ >> (2 * d))] = d
        rec(0, 0)
        return out

    def residual(self, a, z, log2cu, none=False):
        """cbf bits of every depth (consistent, as the encoder writes them) and transform-skip flags of the CU's TUs"""
        P = self.parts[a]
        np_ = 1 << (2 * (log2cu - 2))
        if none:
            return
        for comp, zu, N, bit, tn in cu_tus(P, z, log2cu):
            if comp == 0:
                chroma_here = (log2cu - int(P[zu]["tr_idx"])) > 2 or zu % 4 == 0
                if chroma_here:
                    self.combo = [(self.n_tu >> k) & 1 for k in range(3)]; self.n_tu += 1
                    c = self.combo[0]
                else:
                    c = int(self.rng.rand() < 0.6)
            else:
                c = self.combo[comp]
            if not c:
                continue
            for d in range(bit + 1):                                   # the nodes above the TU
                n = np_ >> (2 * d)
                u0 = z + ((zu - z) // n) * n
                P["cbf"][u0:u0 + n, comp] |= 1 << d
            if comp and bit < int(P[zu]["tr_idx"]):                    # 4x4 chroma of an 8x8 node: the luma depth repeats the parent's bit
                P["cbf"][zu:zu + 4, comp] |= 1 << (bit + 1)
            if N == 4 and self.rng.rand() < 0.35:
                P["tskip"][zu:zu + tn, comp] = 1

    def cu_common(self, x, y, S, mode, ps):
        a = (y // 64) * self.wctu + x // 64
        z = zidx((x & 63) >> 2, (y & 63) >> 2)
        log2cu = S.bit_length() - 1
        np_ = 1 << (2 * (log2cu - 2))
        P = self.parts[a]
        P[z:z + np_] = np.zeros((), PART_DT)
        P["depth"][z:z + np_] = 6 - log2cu; P["pred_mode"][z:z + np_] = mode; P["part_size"][z:z + np_] = ps
        return a, z, log2cu, np_, P

    def intra(self, x, y, S, dirs, tr, cdir=None):
        """dirs: one direction (2Nx2N) or four (NxN, an 8x8 CU)"""
        nxn = len(dirs) == 4
        a, z, log2cu, np_, P = self.cu_common(x, y, S, 1, 3 if nxn else 0)
        P["ref_idx"][z:z + np_] = -1
        P["luma_dir"][z:z + np_] = dirs if nxn else dirs[0]
        if cdir is None:
            cdir = CHROMA_DIRS[self.n_cdir % len(CHROMA_DIRS)]; self.n_cdir += 1
        P["chroma_dir"][z:z + np_] = cdir
        P["tr_idx"][z:z + np_] = self.tr_units(log2cu, tr, nxn)
        self.residual(a, z, log2cu)

    def vector(self, a, cx, cy, px, py, w, h, gt, kind):
        """a vector of the wanted kind for the PU at (px, py), with the next of the 64 chroma phases; what fits() refuses is drawn again"""
        W, H, rng = self.W, self.H, self.rng
        k = self.n_pu
        phx, phy = k & 7, (k >> 3) & 7
        n = self.wctu * self.hctu
        for attempt in range(60):
            tx, ty = px + rng.randint(-6, 7), py + rng.randint(-6, 7)
            if kind in ("decoded", "future"):
                lo, hi = (0, a) if kind == "decoded" else (a + 1, n)
                if lo >= hi:
                    kind = "own_cu"; continue
                b = rng.randint(lo, hi)
                bx, by = (b % self.wctu) * 64, (b // self.wctu) * 64
                bw, bh = min(64, W - bx), min(64, H - by)
                if w > bw or h > bh: continue
                tx, ty = bx + rng.randint(0, bw - w + 1), by + rng.randint(0, bh - h + 1)
            elif kind == "own_cu":
                tx, ty = px + rng.randint(-w + 1, w), py + rng.randint(-h + 1, h)
            elif kind == "margin":
                side = (k // 5 + attempt) % 4
                if side == 0: tx = -rng.randint(1, 70)
                elif side == 1: tx = W - w + rng.randint(1, 70)
                elif side == 2: ty = -rng.randint(1, 70)
                else: ty = H - h + rng.randint(1, 70)
            mvx, mvy = ((tx - px) * 4 & ~7) | phx, ((ty - py) * 4 & ~7) | phy
            if kind == "clip":
                big = [int(rng.randint(1500, 30000)) * (1 if rng.rand() < 0.5 else -1) for _ in range(2)]
                which = (k // 5 + attempt) % 3
                if which != 1: mvx = big[0]
                if which != 0: mvy = big[1]
            c = clip_mv(W, H, cx, cy, mvx, mvy)
            if fits(W, H, px, py, w, h, c[0], c[1], gt):
                return mvx, mvy
        mvx, mvy = phx - 8 * int(rng.randint(0, 2)), phy - 8 * int(rng.randint(0, 2))
        assert fits(W, H, px, py, w, h, mvx, mvy, gt)
        return mvx, mvy

    def inter(self, x, y, S, ps, tr, gt_mode="mix", skip=False, no_residual=False, local=False):
        """gt_mode: "on", "off", "merge" (flagged on a merge PU), "zero" (flagged, all eight values zero), "mix" """
        a, z, log2cu, np_, P = self.cu_common(x, y, S, 0, ps)
        rng = self.rng
        P["inter_dir"][z:z + np_] = 1
        P["tr_idx"][z:z + np_] = 0 if skip else self.tr_units(log2cu, tr)
        P["skip"][z:z + np_] = 1 if skip else 0
        for pu in range(num_pus(ps)):
            ox, oy, w, h = pu_rect(ps, S, pu)
            g = gt_mode if gt_mode != "mix" else ("on", "off", "merge", "zero", "on", "off")[rng.randint(0, 6)]
            merge = 1 if (skip or g == "merge") else int(g == "off" and rng.rand() < 0.3)
            flag = 1 if g in ("on", "merge", "zero") else 0
            gt = np.zeros(8, np.int16)
            if g in ("on", "merge"):
                r = (2, min(w, h) // 2, 40, 300)[rng.randint(0, 4)]
                while not gt.any(): gt = rng.randint(-r, r + 1, 8).astype(np.int16)
            eff = g == "on"
            kind = MV_KINDS[(0, 3, 0, 1, 2, 0, 4, 3, 0, 2)[self.n_pu % 10]]
            if w * h >= 256 and rng.rand() < 0.7:
                kind = "decoded"                                          # a large block of sentinel samples predicts a large block of zeros: keep most of those small
            if local:                                                     # some tens of samples up and to the left, four at most down or to the right: the eight CTUs around
                k = self.n_pu
                dx, dy = -int(rng.randint(-4, 41)), -int(rng.randint(-4, 41))
                if rng.rand() < 0.8:                                      # mostly clear of the PU itself, whose samples are still the sentinel
                    if h <= 40: dy = -int(rng.randint(h, 41))
                    elif w <= 40: dx = -int(rng.randint(w, 41))
                mv = ((dx * 4 & ~7) | (k & 7), (dy * 4 & ~7) | ((k >> 3) & 7))
                assert fits(self.W, self.H, x + ox, y + oy, w, h, mv[0], mv[1], eff)
                if k % 9 == 4 and w * h <= 256:                           # and some into the next CTU to the right or the one below: still the sentinel, in every schedule
                    mv = ((64 * 4) | (k & 7), mv[1]) if (k // 9) % 2 and x + 128 <= self.W else (mv[0], (64 * 4) | ((k >> 3) & 7)) if y + 128 <= self.H else mv
                    assert fits(self.W, self.H, x + ox, y + oy, w, h, mv[0], mv[1], eff)
            else:
                mv = self.vector(a, x, y, x + ox, y + oy, w, h, eff, kind)
            self.n_pu += 1
            for yy in range(oy, oy + h, 4):
                for xx in range(ox, ox + w, 4):
                    zi = zidx(((x & 63) + xx) >> 2, ((y & 63) + yy) >> 2)
                    P["mv"][zi] = mv; P["merge_flag"][zi] = merge; P["gt_flag"][zi] = flag; P["gt"][zi] = gt
        self.residual(a, z, log2cu, none=skip or no_residual)

    # ---- layout: the wanted CUs packed bottom-up into quadtrees, the trees dealt to the whole CTUs ----
    def layout(self, wanted, filler):
        """wanted: {size: [put(x, y), ...]}; filler(x, y): an 8x8 CU where nothing is wanted"""
        rng = self.rng
        items = []                                                       # (size, put | None (fillers) | [four items of half the size])
        for S in (8, 16, 32, 64):
            items += [(S, f) for f in wanted.get(S, [])]
            items = [items[k] for k in rng.permutation(len(items))]
            if S == 64:
                break
            items += [(S, None)] * (-len(items) % 4)
            items = [(2 * S, items[k:k + 4]) for k in range(0, len(items), 4)]

        def place(item, x, y):
            S, f = item
            if isinstance(f, list):
                for k, sub in enumerate(f): place(sub, x + (k & 1) * (S // 2), y + (k >> 1) * (S // 2))
            elif f is None:
                for yy in range(y, y + S, 8):
                    for xx in range(x, x + S, 8): filler(xx, yy)
            else:
                f(x, y)
        whole = [(cx * 64, cy * 64) for cy in range(self.H // 64) for cx in range(self.W // 64)]
        assert len(items) <= len(whole), (len(items), len(whole))
        items += [(64, None)] * (len(whole) - len(items))
        items = [items[k] for k in rng.permutation(len(items))]
        for a in range(self.wctu * self.hctu):
            x, y = (a % self.wctu) * 64, (a // self.wctu) * 64
            if x + 64 <= self.W and y + 64 <= self.H:
                place(items[whole.index((x, y))], x, y)
            else:
                for yy in range(y, min(y + 64, self.H), 8):
                    for xx in range(x, min(x + 64, self.W), 8): filler(xx, yy)


def _intra_all(B):
    rng = B.rng
    w = {64: [], 32: [], 16: [], 8: []}
    w[64] += [lambda x, y: B.intra(x, y, 64, [34], 1), lambda x, y: B.intra(x, y, 64, [9], 2), lambda x, y: B.intra(x, y, 64, [1], "mix")]
    for d in range(35):
        w[32].append(lambda x, y, d=d: B.intra(x, y, 32, [d], 0))
        w[16].append(lambda x, y, d=d: B.intra(x, y, 16, [d], 0))
        w[8].append(lambda x, y, d=d: B.intra(x, y, 8, [d], 0))
    for t, d in ((1, 3), (2, 21), (3, 13), (3, 29), ("mix", 0), ("mix", 17)):
        w[32].append(lambda x, y, t=t, d=d: B.intra(x, y, 32, [d], t))
    for t, d in ((1, 5), (2, 33), (2, 11), ("mix", 26), ("mix", 2)):
        w[16].append(lambda x, y, t=t, d=d: B.intra(x, y, 16, [d], t))
    for k in range(9):                                                    # NxN: 36 units, every direction on a 4x4 TU
        w[8].append(lambda x, y, k=k: B.intra(x, y, 8, [(4 * k + j) % 35 for j in range(4)], 1))
    for d in (0, 1, 10, 26, 34, 6, 22):
        w[8].append(lambda x, y, d=d: B.intra(x, y, 8, [d], 1))           # 2Nx2N 8x8 over four 4x4 TUs
    B.layout(w, lambda x, y: B.intra(x, y, 8, [int(rng.randint(0, 35))], int(rng.randint(0, 2))))


def _inter_all(B):
    rng = B.rng
    w = {64: [], 32: [], 16: [], 8: []}
    gts = ("on", "off", "merge", "zero")
    for ps in INTER_PART_SIZES:
        w[64].append(lambda x, y, ps=ps: B.inter(x, y, 64, ps, 1 + ps % 3, gts[ps % 4] if ps < 4 else "mix"))
        for k in range(2):
            w[32].append(lambda x, y, ps=ps, k=k: B.inter(x, y, 32, ps, (ps + 2 * k) % 4, ("on", "mix")[k]))
            w[16].append(lambda x, y, ps=ps, k=k: B.inter(x, y, 16, ps, (ps + k) % 3, ("on", "mix")[k]))
    for ps in range(3):
        for k in range(4):
            w[8].append(lambda x, y, ps=ps, k=k: B.inter(x, y, 8, ps, k % 2, ("on", "on", "off", "mix")[k]))
    for S in (32, 16, 16, 8, 8):
        w[S].append(lambda x, y, S=S: B.inter(x, y, S, 0, 0, "off", skip=True))
    for S, ps in ((16, 1), (8, 0), (32, 6)):
        w[S].append(lambda x, y, S=S, ps=ps: B.inter(x, y, S, ps, 0, "mix", no_residual=True))
    for S, n in ((32, 3), (16, 8), (8, 16)):
        for k in range(n):
            w[S].append(lambda x, y, S=S, k=k: B.intra(x, y, S, [int(rng.randint(0, 35))], "mix" if k % 2 else 0))
    w[8] += [lambda x, y, k=k: B.intra(x, y, 8, [(7 * k + j * 9) % 35 for j in range(4)], 1) for k in range(4)]

    def filler(x, y):
        if rng.rand() < 0.4: B.intra(x, y, 8, [int(rng.randint(0, 35))], int(rng.randint(0, 2)))
        else: B.inter(x, y, 8, int(rng.randint(0, 3)), int(rng.randint(0, 2)))
    B.layout(w, filler)


def _mixed_local(B):
    rng = B.rng

    def cu(x, y, S):
        if S > 8 and rng.rand() < (0.75 if S == 64 else 0.45):
            for k in range(4): cu(x + (k & 1) * (S // 2), y + (k >> 1) * (S // 2), S // 2)
        elif rng.rand() < 0.45:
            nxn = S == 8 and rng.rand() < 0.3
            B.intra(x, y, S, [int(v) for v in rng.randint(0, 35, 4 if nxn else 1)], "mix")
        else:
            B.inter(x, y, S, int(rng.randint(0, 3)) if S == 8 else INTER_PART_SIZES[rng.randint(0, 7)], "mix", local=True)
    for a in range(B.wctu * B.hctu):
        cu((a % B.wctu) * 64, (a // B.wctu) * 64, 64)


@functools.lru_cache(maxsize=None)
def syntax(kind):
    W, H = SIZES[kind]
    B = _Builder(W, H, {"intra_all": 101, "inter_all": 202, "mixed_local": 303}[kind])
    {"intra_all": _intra_all, "inter_all": _inter_all, "mixed_local": _mixed_local}[kind](B)
    B.parts.setflags(write=False)
    return B.parts


def fill_levels(parts, bd, qps, seed):
    """levels of every TU whose cbf is set: one of four shapes, one of three magnitudes (fewer large ones the coarser the quantiser: large levels saturate).
    Returns (levels, the (shape, magnitude) pairs made)"""
    rng = np.random.RandomState(seed)
    levels = np.zeros((parts.shape[0], 6144), np.int32)
    made = set()
    for a, z, log2cu in cus(parts):
        P = parts[a]
        for comp, zu, N, bit, tn in cu_tus(P, z, log2cu):
            if not (int(P[zu]["cbf"][comp]) >> bit) & 1:
                continue
            q = qps[comp]
            pm = (0.35, 0.45, 0.2) if q < 15 else (0.6, 0.3, 0.1) if q < 40 else (0.9, 0.08, 0.02)
            mag = int(rng.choice(3, p=pm)); shape = int(rng.choice(4, p=(0.25, 0.15, 0.35, 0.25)))
            bound = level_bound(bd, q, N)
            top = (3, 255, min(32767, bound))[mag]
            v = np.zeros(N * N, np.int64)
            idx = {0: [0], 1: [N * N - 1], 2: rng.choice(N * N, max(1, N * N // 16), replace=False), 3: np.arange(N * N)}[shape]
            v[idx] = rng.randint(1, top + 1, len(idx)) * rng.choice((-1, 1), len(idx))
            if mag == 2:                                                  # the ends of the range themselves
                v[idx[0]] = top if rng.rand() < 0.5 else -min(32768, bound)
            base = 16 * zu if comp == 0 else (4096 if comp == 1 else 5120) + 4 * zu
            levels[a, base:base + N * N] = v
            made.add((SHAPES[shape], MAGS[mag]))
    return levels, made


@functools.lru_cache(maxsize=None)
def make_case(name):
    kind, bd, plain, qp, cb, cr = CASES[name]
    W, H = SIZES[kind]
    parts = syntax(kind)
    qps = (qp + 6 * (bd - 8), chroma_qp_scaled(qp, cb, bd), chroma_qp_scaled(qp, cr, bd))
    levels, made = fill_levels(parts, bd, qps, sum(ord(c) for c in name))
    case = dict(name=name, W=W, H=H, bd=bd, plain=plain, qp=qp, cb_off=cb, cr_off=cr, parts=parts, levels=levels)
    case["coverage"] = coverage(case) | {("level",) + m for m in made}
    return case


def coverage(case):
    """what the case contains, read from its parts: a set of tuples"""
    W, H, parts = case["W"], case["H"], case["parts"]
    wctu = (W + 63) // 64
    cov = set()
    for a, z, log2cu in cus(parts):
        P = parts[a]; S = 1 << log2cu; p0 = P[z]
        x4, y4 = zpos(z); cx, cy = (a % wctu) * 64 + 4 * x4, (a // wctu) * 64 + 4 * y4
        intra = p0["pred_mode"] == 1
        kind = "intra" if intra else "inter"
        cov.add((kind, "depth", int(p0["depth"])))
        tus = cu_tus(P, z, log2cu)
        for comp, zu, N, bit, tn in tus:
            c = (int(P[zu]["cbf"][comp]) >> bit) & 1
            if comp == 0:
                cov.add((kind, "tr_idx", S, int(P[zu]["tr_idx"])))
                if intra: cov.add(("intra", "luma_dir", N, int(P[zu]["luma_dir"])))
                if N == 4 and S > 8: cov.add((kind, "split_to_4x4", S))
            if c and P[zu]["tskip"][comp]:
                cov.add((kind, "tskip", "luma" if comp == 0 else "chroma"))
        lum = [t for t in tus if t[0] == 0]
        for comp, zu, N, bit, tn in lum:                                 # the luma TUs that carry chroma
            ch = [t for t in tus if t[0] and t[1] == zu]
            if ch:
                cov.add((kind, "cbf") + tuple((int(P[zu]["cbf"][t[0]]) >> t[3]) & 1 for t in [(comp, zu, N, bit, tn)] + ch))
        if intra:
            cov.add(("intra", "chroma_dir", int(p0["chroma_dir"])))
            if p0["part_size"] == 3 and len(set(int(P[z + k]["luma_dir"]) for k in range(4))) == 4: cov.add(("intra", "nxn_four_directions"))
            if S == 8 and p0["part_size"] == 0 and p0["tr_idx"] == 1: cov.add(("intra", "8x8_2Nx2N_tr1"))
            continue
        ps = int(p0["part_size"])
        cov.add(("inter", "part_size", S, ps))
        if p0["skip"]: cov.add(("inter", "skip"))
        elif not any(P["cbf"][z:z + (1 << (2 * (log2cu - 2)))].ravel()): cov.add(("inter", "root_cbf_0"))
        for pu in range(num_pus(ps)):
            ox, oy, w, h = pu_rect(ps, S, pu)
            p = P[zidx(((cx & 63) + ox) >> 2, ((cy & 63) + oy) >> 2)]
            raw = (int(p["mv"][0]), int(p["mv"][1]))
            mv = clip_mv(W, H, cx, cy, *raw)
            cov.add(("inter", "phase_luma", mv[0] & 3, mv[1] & 3)); cov.add(("inter", "phase_chroma", mv[0] & 7, mv[1] & 7))
            eff = bool(p["gt_flag"]) and not p["merge_flag"] and bool(np.any(p["gt"]))
            cov.add(("inter", "gt", "on" if eff else "off"))
            if eff: cov.add(("inter", "gt_pu", w, h))
            if p["gt_flag"] and p["merge_flag"] and np.any(p["gt"]): cov.add(("inter", "gt_flag_on_merge"))
            if p["gt_flag"] and not p["merge_flag"] and not np.any(p["gt"]): cov.add(("inter", "gt_flag_all_zero"))
            # where the block the vector points at lies
            tx, ty = cx + ox + (mv[0] >> 2), cy + oy + (mv[1] >> 2)
            if mv != raw: cov.add(("inter", "mv", "clip"))
            if tx < 0: cov.add(("inter", "mv", "margin_left"))
            if tx + w > W: cov.add(("inter", "mv", "margin_right"))
            if ty < 0: cov.add(("inter", "mv", "margin_top"))
            if ty + h > H: cov.add(("inter", "mv", "margin_bottom"))
            if tx < cx + S and tx + w > cx and ty < cy + S and ty + h > cy: cov.add(("inter", "mv", "own_cu"))
            if 0 <= tx and tx + w <= W and 0 <= ty and ty + h <= H:
                ctus = set((yy // 64) * wctu + xx // 64 for yy in (ty, ty + h - 1) for xx in (tx, tx + w - 1))
                if max(ctus) < a: cov.add(("inter", "mv", "decoded"))
                if min(ctus) > a: cov.add(("inter", "mv", "future"))
    return cov
