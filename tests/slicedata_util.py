"""Helpers of the slice-data tests (tests/test_slicedata_cpu.py, tests/test_gpu_slicedata.py) and of tools/make_golden_slicedata.py: the fixture cases, the cut of a
bitstream into the RBSP of its slices, and the ctypes view of hop_slice_data_params.

tests/golden/slice_data.npz holds, per case, the whole .bin the unmodified reference encoder wrote ("<key>/bin"), the options it ran with ("<key>/args") and, per
configuration, the byte length of the first picture's slice header ("header/<config>").  The slice data of a picture is the tail of its VCL NAL unit's RBSP."""
import ctypes
import os

import numpy as np

from hoputil import PIC_CASES, ROOT, hop_encoder_args, lenslet, pic_case_args, pic_case_input, sharp_frame

FIXTURE = os.path.join(ROOT, "tests", "golden", "slice_data.npz")


def _raw(planes):
    return b"".join(p.astype(np.uint8).tobytes() for p in planes)


def _hop(W, H, frame, **over):
    return {"W": W, "H": H, "frames": 1, "frame": frame, "args": hop_encoder_args(W, H, **over), "over": over}


def slice_cases():
    """key -> {W, H, frames, args (the encoder's options), rows (substreams per picture), sao, plain (bit depth, qp) or None, mi, config (the header-length class),
    input (the .yuv bytes), pictures (per frame Y, Cb, Cr)}"""
    out = {}
    for key, c in PIC_CASES.items():                                        # (a)
        bd = c["plain"][0] if "plain" in c else 8
        pics = [lenslet(c["W"], c["H"], c.get("pitch", 16), c["seed"] + 100 * f, bitdepth=bd) for f in range(c["frames"])]
        out[key] = {"W": c["W"], "H": c["H"], "frames": c["frames"], "args": pic_case_args(c), "over": c["over"], "plain": c.get("plain"), "input": pic_case_input(c), "pictures": pics}
    extra = {
        "64x64_sharp77": _hop(64, 64, sharp_frame(64, 64, 77)),                                                                  # (b) intra NxN, transform skip
        "64x192_wpp": _hop(64, 192, lenslet(64, 192, 16, 3), WaveFrontSynchro=1, WaveFrontSubstreams=3),                          # (c) one CTU wide: no synchronisation
        "128x256_wpp": _hop(128, 256, lenslet(128, 256, 16, 3), WaveFrontSynchro=1, WaveFrontSubstreams=4),                       #     two wide: the point is the row's last CTU
        "64x64_raster_sao0": _hop(64, 64, lenslet(64, 64, 16, 1234), SAO=0),                                                      # (d) parts and levels alone
        "192x128_wpp_sao0": _hop(192, 128, lenslet(192, 128, 16, 7), SAO=0, WaveFrontSynchro=1, WaveFrontSubstreams=2),
        "64x64_sharp77_sao0": _hop(64, 64, sharp_frame(64, 64, 77), SAO=0),
    }
    for key, c in extra.items():
        c.update({"plain": None, "input": _raw(c["frame"]), "pictures": [c["frame"]]})
        out[key] = c
    for key, c in out.items():
        o = c["over"]
        c["rows"] = o.get("WaveFrontSubstreams", 1) if o.get("WaveFrontSynchro") else 1
        c["wpp"] = 1 if o.get("WaveFrontSynchro") else 0
        c["sao"] = o.get("SAO", 1)
        c["mi"] = o.get("mi", 16)
        c["qp"] = c["plain"][1] if c["plain"] else 32
        c["bd"] = c["plain"][0] if c["plain"] else 8
        c["slice_type"] = 2 if c["plain"] else 3
        c["config"] = ("plain%d" % c["bd"] if c["plain"] else "hop") + ("" if c["sao"] else "_sao0") + ("_mi15" if c["mi"] == 15 else "")
    return out


# ---- the bitstream: NAL units at their start codes, the VCL ones without emulation prevention ----
def nal_units(data):
    """the NAL units of an Annex B stream (bytes after each 00 00 01 start code, trailing zero bytes of the next start code's prefix cut)"""
    pos, out = [], []
    i = data.find(b"\x00\x00\x01")
    while i >= 0:
        pos.append(i)
        i = data.find(b"\x00\x00\x01", i + 3)
    for k, p in enumerate(pos):
        end = pos[k + 1] if k + 1 < len(pos) else len(data)
        u = data[p + 3:end]
        if k + 1 < len(pos) and u.endswith(b"\x00"):                        # the zero_byte of a four-byte start code belongs to the next unit
            u = u[:-1]
        out.append(u)
    return out


def strip_emulation_prevention(u):
    """RBSP of a NAL unit: every 03 that follows 00 00 removed"""
    out, zeros = bytearray(), 0
    for b in u:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def slice_payloads(data):
    """per picture of the stream the RBSP of its slice NAL unit behind the two header bytes (slice header, then slice data); VCL: nal_unit_type 0..31"""
    return [strip_emulation_prevention(u)[2:] for u in nal_units(bytes(data)) if ((u[0] >> 1) & 0x3F) < 32]


class SliceDataParams(ctypes.Structure):                                     # hop_slice_data_params
    _fields_ = [(n, ctypes.c_int32) for n in ("qp", "slice_type", "wpp", "plain_intra", "sao_luma", "sao_chroma", "mi_size")]


def params_of(c, sao_luma=None, sao_chroma=None):
    on = c["sao"] if sao_luma is None else sao_luma
    return SliceDataParams(c["qp"], c["slice_type"], c["wpp"], 1 if c["plain"] else 0, on, c["sao"] if sao_chroma is None else sao_chroma, c["mi"])


def sao_lambdas(qp):
    """TEncSlice::initEncSlice (TLibEncoder/TEncSlice.cpp:442-468): Y, Cb, Cr with the chroma weights"""
    scale = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
             29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51]
    lam = 0.57 * 2.0 ** ((qp - 12) / 3.0)
    w = 2.0 ** ((qp - scale[min(57, max(0, qp))]) / 3.0)
    return [lam, lam / w, lam / w]


def load_fixture():
    return np.load(FIXTURE)


def fixture_slice_data(G, key, picture, n_bytes):
    """the last n_bytes of the picture's slice payload, and the payload's length"""
    p = slice_payloads(G[key + "/bin"].tobytes())[picture]
    return p[len(p) - n_bytes:], len(p)


def check_header(G, c, picture, header_bytes):
    """what lies in front of the matched slice data must be a slice header and nothing more, so that a too-short output cannot pass as a suffix: the first picture of a
    one-substream case has exactly the stored header of its configuration ("header/<config>" without the wavefront's share: the configurations differ in SAO, bit depth
    and micro-image size only); a later picture may add the bytes of its picture order count (at most 2); a wavefront picture adds its entry points: two ue(v) of at
    most 2 bytes together with the alignment, and at most 4 bytes per offset"""
    base = int(G["header/" + c["config"]][0])
    extra = (2 if picture else 0) + (2 + 4 * (c["rows"] - 1) if c["rows"] > 1 else 0)
    assert base <= header_bytes <= base + extra, (c["config"], picture, header_bytes, base, extra)
