#!/usr/bin/env python3
"""tools/make_golden_qps.py -- tests/golden/stream_qps.npz: the bitstreams the UNMODIFIED reference encoder (oracle/_ref/TAppEncoderRef, built by build() where the
reference tree is present) writes for two of the slice-data cases at QPs other than the 32 every other fixture of the repository is coded at:

  192x128_wpp     (HOP configuration, wavefront, 3 x 2 CTUs)        -q 22, 27, 37
  136x72_plain8   (plain intra, 8 bit, partial CTUs right and below) -q 22, 37

The QP-32 stream of either case is tests/golden/slice_data.npz's and is not stored again.  Per stream the .bin is kept ("<key>/q<qp>/bin", a few hundred bytes to
2 KB), per case the options its streams were written with ("<key>/args", once: they differ in the value behind -q alone, which is stored as %d).
tests/picture_qps_util.py reads the fixture.

The tool asserts what the tests lean on (tests/test_picture_qps_cpu.py, tests/test_gpu_picture_qps.py decode and write the streams of a case side by side, one call for
all QPs, and such a call takes ONE pair of slice SAO flags):
  * all streams of a case, the QP-32 one included, carry the same two slice SAO flags -- the reference switches neither at any of these QPs, so no QP had to be moved;
  * their slice-data bytes are pairwise different (a table index that picked the wrong QP cannot go unnoticed);
  * the streams shrink as the QP rises.

Run in the build container, after build()."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402
import stream_read_util as R  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_qps.npz")
QPS = {"192x128_wpp": (22, 27, 37), "136x72_plain8": (22, 37)}


def encode(c, args):
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "in.yuv"), "wb").write(c["input"])
        for attempt in range(6):                 # (the reference's GT search reads past its reference picture buffer; now and then that kills the process: tools/make_golden_slicedata.py)
            r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "TAppEncoderRef")] + args, cwd=td, capture_output=True, text=True)
            if r.returncode != -11: break
        assert r.returncode == 0, r.stdout[-2000:]
        return open(os.path.join(td, "s.bin"), "rb").read()


def with_qp(args, qp):
    at = args.index("-q")
    return args[:at + 1] + [str(qp)] + args[at + 2:]


def main():
    hp = R.hophip()
    cases = U.slice_cases()
    G = U.load_fixture()
    out = {}
    for key, qps in QPS.items():
        c = cases[key]
        assert c["qp"] == 32 and c["frames"] == 1
        bins = {32: G[key + "/bin"].tobytes()}
        for qp in qps:
            args = with_qp(c["args"], qp)
            bins[qp] = encode(c, args)
            out["%s/q%d/bin" % (key, qp)] = np.frombuffer(bins[qp], np.uint8)
        out[key + "/args"] = np.frombuffer(" ".join(with_qp(c["args"], "%d")).encode(), np.uint8)
        read = {qp: hp.access_unit_read_host(b, None) for qp, b in bins.items()}          # (info, rbsp, sizes, digest)
        for qp, (info, rbsp, sizes, digest) in read.items():
            s, s32 = info.params.slice, read[32][0].params.slice
            assert s.qp == qp, (key, qp, s.qp)
            assert (s.sao_luma, s.sao_chroma) == (s32.sao_luma, s32.sao_chroma), "%s: the reference switches an SAO flag at QP %d: take the nearest QP where it does not" % (key, qp)
        order = sorted(bins)
        for i, a in enumerate(order):
            for b in order[i + 1:]:
                assert read[a][1] != read[b][1], (key, a, b)
        for a, b in zip(order[:-1], order[1:]):
            assert len(bins[a]) > len(bins[b]) and len(read[a][1]) > len(read[b][1]), (key, a, b, len(bins[a]), len(bins[b]))
        print(key, {qp: len(bins[qp]) for qp in order}, "bytes; SAO flags", (read[32][0].params.slice.sao_luma, read[32][0].params.slice.sao_chroma), flush=True)
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
