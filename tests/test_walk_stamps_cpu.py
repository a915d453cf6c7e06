"""CPU: the diagnostic build with the candidate walks' stage stamps (libhophip_stamps.so, hop_walk_stamps_* of include/hophip.h) as a binding sees it.

The build leaves two libraries side by side -- the product, and the same objects with csrc/k_cabac.hip compiled once more with -DHOP_WALK_STAMPS=1 -- that export the same
hop_* functions, so that a program switches between them by the path alone (HOP_LIB for hophip.py).  No GPU call is made here; what the stamps record is
tests/test_gpu_walk_stamps.py's."""
import ctypes
import os
import subprocess
import sys

from hoputil import ROOT

sys.path.insert(0, os.path.join(ROOT, "hevc-hop_amd"))
import hophip  # noqa: E402

PRODUCT = os.path.join(ROOT, "hevc-hop_amd", "libhophip.so")
STAMPS = os.path.join(ROOT, "hevc-hop_amd", "libhophip_stamps.so")


def _exports(path):
    return {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", path], text=True).splitlines() if " T hop_" in ln}


def test_both_libraries_are_built():
    assert os.path.exists(PRODUCT) and os.path.exists(STAMPS)
    assert hophip.STAMPS_LIB_PATH == STAMPS


def test_both_libraries_export_the_same_functions():
    prod, st = _exports(PRODUCT), _exports(STAMPS)
    assert prod == st, sorted(prod ^ st)
    assert {"hop_walk_stamps_read", "hop_walk_stamps_reset", "hop_walk_stamps_probe", "hop_walk_stamps_stage_name"} <= prod


def test_stage_names_are_distinct_and_end_where_the_enum_ends():
    for path in (PRODUCT, STAMPS):
        L = ctypes.CDLL(path)
        names = hophip.walk_stamps_stage_names(L)
        assert len(names) == hophip.HOP_WS_COUNT == 15 and all(names) and len(set(names)) == len(names), names
        assert names[hophip.HOP_WS_LEAF_FORWARD] == "LEAF_FORWARD" and names[hophip.HOP_WS_LEAF_RDOQ] == "LEAF_RDOQ" and names[hophip.HOP_WS_OTHER] == "OTHER"
        assert L.hop_walk_stamps_stage_name(-1) is None and L.hop_walk_stamps_stage_name(hophip.HOP_WS_COUNT) is None
    # the header's enum ends where the binding's does
    hdr = open(os.path.join(ROOT, "include", "hophip.h")).read()
    body = hdr[hdr.index("HOP_WS_LEAF_FORWARD = 0"):hdr.index("HOP_WS_COUNT\n")]
    assert body.count("HOP_WS_") == hophip.HOP_WS_COUNT
    assert [("HOP_WS_" + n) in body for n in names] == [True] * len(names)


def test_binding_struct_size_is_the_librarys():
    for path in (PRODUCT, STAMPS):
        L = ctypes.CDLL(path)
        L.hop_sizeof.argtypes = [ctypes.c_char_p]
        assert L.hop_sizeof(b"hop_walk_stamps_total") == ctypes.sizeof(hophip.WalkStampsTotal) == 32
    assert hophip.MIRRORS["hop_walk_stamps_total"] is hophip.WalkStampsTotal
