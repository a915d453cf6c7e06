#!/usr/bin/env python3
"""tools/quant_flat_dump.py OUT -- the blocks tools/quant_flat_check.cpp runs through hop_quant_flat_tu_host, with the levels and sums expected of it: the 400 + 600
blocks of tests/golden/quant_flat.npz and quant_flat_sbh.npz (quantised by the reference's own xQuant with RDOQ off) and the crafted blocks of tests/quant_mode_util.py
under the three scans and both rounding offsets (expected: the oracle's hop_o_quant_flat_sbh).

The file: int32 0x51464C54, int32 count; per block int32 bit_depth, qp_scaled, i_slice, log2_size, sign_hide, scan_idx, abs_sum, then N*N int32 coefficients and N*N
int32 expected levels."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quant_mode_util as Q  # noqa: E402
from goldutil import load  # noqa: E402


def blocks():
    g = load("quant_flat.npz")
    for N, bd, qp, isI, asum, off in g["par"]:
        N, off = int(N), int(off)
        yield (int(bd), int(qp), int(isI), N.bit_length() - 1, 0, 0, int(asum)), g["src"][off:off + N * N], g["out"][off:off + N * N]
    g = load("quant_flat_sbh.npz")
    for N, bd, qp, isI, asum, off, scan in g["par"]:
        N, off = int(N), int(off)
        yield (int(bd), int(qp), int(isI), N.bit_length() - 1, 1, int(scan), int(asum)), g["src"][off:off + N * N], g["out"][off:off + N * N]
    for name, (N, qp, values) in Q.crafted().items():
        for scan in (0, 1, 2):
            for is_i in (0, 1):
                coef = Q.in_scan_order(N, scan, values)
                want, asum = Q.oracle_flat_sbh(coef, 8, qp, is_i, scan)
                yield (8, qp, is_i, N.bit_length() - 1, 1, scan, asum), coef.ravel(), want.ravel()


def main():
    all_blocks = list(blocks())
    with open(sys.argv[1], "wb") as f:
        f.write(np.array([0x51464C54, len(all_blocks)], "<i4").tobytes())
        for head, src, want in all_blocks:
            f.write(np.array(head, "<i8").astype("<i4").tobytes() + np.asarray(src).astype("<i4").tobytes() + np.asarray(want).astype("<i4").tobytes())
    print("wrote", sys.argv[1], len(all_blocks), "blocks")


if __name__ == "__main__":
    main()
