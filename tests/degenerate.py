"""Degenerate pictures -- TEST INFRASTRUCTURE.  Noise-free, deterministic content on which many candidates of a search have exactly the same cost (flat areas, exact
repeats) or on which samples sit at the ends of the range (two-level pictures, clipped ramps): what the black corners, clipped highlights and the exactly repeating
micro-image grid of real lenslet frames do to the searches, and what the noisy synthetic lenslets of hoputil never do.  Pure numpy; every picture is (Y, Cb, Cr) int16,
4:2:0.  Chroma: mid-grey for flat() and tile(), the luma subsampled for the others.  The pictures are not stored in tests/golden/degenerate.npz: they are regenerated here
and pinned by the CRCs the golden carries."""
import zlib

import numpy as np


def top_of(bd):
    return (1 << bd) - 1


def mid_of(bd):
    return 1 << (bd - 1)


def _grey(W, H, bd):
    return np.full((H // 2, W // 2), mid_of(bd), np.int16)


def _sub(Y):
    return np.ascontiguousarray(Y[::2, ::2])


def flat(W, H, v, bd=8):
    """every luma sample v; v may be "mid" or "top" """
    v = {"mid": mid_of(bd), "top": top_of(bd)}.get(v, v)
    return np.full((H, W), int(v), np.int16), _grey(W, H, bd), _grey(W, H, bd)


def tile(W, H, p, seed, bd=8):
    """a seeded random p x p block repeated exactly"""
    blk = np.random.default_rng(seed).integers(0, top_of(bd) + 1, (p, p)).astype(np.int16)
    Y = np.ascontiguousarray(np.tile(blk, ((H + p - 1) // p, (W + p - 1) // p))[:H, :W])
    return Y, _grey(W, H, bd), _grey(W, H, bd)


def stripes(W, H, k, bd=8):
    """vertical bars of 0 and top, k samples wide"""
    row = ((np.arange(W) // k) & 1).astype(np.int16) * top_of(bd)
    Y = np.ascontiguousarray(np.broadcast_to(row, (H, W)))
    return Y, _sub(Y), _sub(Y)


def checker(W, H, k, bd=8):
    """k x k squares of 0 and top"""
    yy, xx = np.mgrid[0:H, 0:W]
    Y = ((((yy // k) + (xx // k)) & 1) * top_of(bd)).astype(np.int16)
    return Y, _sub(Y), _sub(Y)


def binary(W, H, seed, bd=8):
    """0 or top per sample, seeded"""
    Y = (np.random.default_rng(seed).integers(0, 2, (H, W)) * top_of(bd)).astype(np.int16)
    return Y, _sub(Y), _sub(Y)


def ramp(W, H, bd=8):
    """a horizontal ramp of twice the range over the picture's width, clipped at both ends: the left quarter is 0, the right quarter top"""
    t = top_of(bd)
    row = np.clip((np.arange(W) * 4 * t) // (2 * W) - t // 2, 0, t).astype(np.int16)
    Y = np.ascontiguousarray(np.broadcast_to(row, (H, W)))
    return Y, _sub(Y), _sub(Y)


def inverted(pic, bd=8):
    return tuple((top_of(bd) - a).astype(np.int16) for a in pic)


PICTURES = {
    "flat_mid": lambda W, H, bd: flat(W, H, "mid", bd), "flat_0": lambda W, H, bd: flat(W, H, 0, bd), "flat_top": lambda W, H, bd: flat(W, H, "top", bd),
    "tile8": lambda W, H, bd: tile(W, H, 8, 8, bd), "tile15": lambda W, H, bd: tile(W, H, 15, 15, bd), "tile16": lambda W, H, bd: tile(W, H, 16, 16, bd),
    "stripes1": lambda W, H, bd: stripes(W, H, 1, bd), "stripes3": lambda W, H, bd: stripes(W, H, 3, bd),
    "checker1": lambda W, H, bd: checker(W, H, 1, bd), "checker4": lambda W, H, bd: checker(W, H, 4, bd), "checker8": lambda W, H, bd: checker(W, H, 8, bd),
    "binary": lambda W, H, bd: binary(W, H, 5, bd), "ramp": lambda W, H, bd: ramp(W, H, bd),
}


def picture(name, W, H, bd=8):
    return PICTURES[name](W, H, bd)


def pic_crc(pic):
    """one CRC over the three planes (as int16) of a picture: what tests/golden/degenerate.npz pins the regenerated pictures with"""
    c = 0
    for a in pic:
        c = zlib.crc32(np.ascontiguousarray(a, np.int16).tobytes(), c)
    return c & 0xFFFFFFFF


# ---- the sets of tests/golden/degenerate.npz (oracle/make_golden25.py) ----
ME_W, ME_H = 320, 256
ME_PICTURES = ["flat_mid", "flat_0", "flat_top", "tile8", "tile15", "stripes3", "checker4"]
PRED_PICTURES = ["flat_top", "flat_0", "stripes1", "stripes3", "checker1", "binary"]
INTRA_W, INTRA_H = 256, 192
INTRA_RECS = ["binary", "flat_top", "flat_0", "checker8", "ramp"]
# key, picture, W, H, WaveFrontSynchro
SPINE_FRAMES = [("128x64_flat_mid", "flat_mid", 128, 64, False), ("128x64_flat_0", "flat_0", 128, 64, False), ("128x64_flat_top", "flat_top", 128, 64, False),
                ("128x64_checker4", "checker4", 128, 64, False), ("128x64_tile16", "tile16", 128, 64, False), ("136x72_flat_mid", "flat_mid", 136, 72, False),
                ("128x128_tile16_wpp", "tile16", 128, 128, True)]
