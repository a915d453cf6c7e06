#!/usr/bin/env python3
"""tools/make_golden_rdoq0.py -- tests/golden/stream_rdoq0.npz: the bitstreams the UNMODIFIED reference encoder (oracle/_ref/TAppEncoderRef, built by build() where the
reference tree is present) writes for three of the slice-data cases with RDOQ switched off, the options of the case with --RDOQ / --RDOQTS appended:

  64x64_raster       (HOP configuration, one CTU)                                      --RDOQ=0 --RDOQTS=0
  136x72_plain10     (plain intra, 10 bit, an I slice: the quantiser's offset is 171)   --RDOQ=0 --RDOQTS=0
  448x192_seed3_mi15_wpp (HOP configuration, --MIsize=15, WaveFrontSynchro, 7 x 3 CTUs; the one wavefront case whose picture holds transform-skip units that RDOQTS changes)
                                                                                         --RDOQ=0 --RDOQTS=0   and   --RDOQ=1 --RDOQTS=0

The RDOQ-on stream of every case is tests/golden/slice_data.npz's and is not stored again.  Per stream "<case>_rdoq<r><t>/bin" (a few hundred bytes to 3 KB) and
"<case>_rdoq<r><t>/args" (the options).  tests/quant_mode_util.py reads the fixture.

The tool asserts what the tests lean on (tests/test_quant_mode_cpu.py re-checks it):
  * the switch changes no syntax: every NAL unit but the slice's and the picture-hash SEI equals the RDOQ-on stream's;
  * the slice NAL unit differs from the RDOQ-on one -- a case whose stream does not change shows nothing and has to be replaced;
  * the mixed stream (RDOQ on, RDOQTS off) differs from both pure ones: its picture holds transform-skip units and others.

Run in the build container, after build()."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_rdoq0.npz")
MODES = {"64x64_raster": ((0, 0),), "136x72_plain10": ((0, 0),), "448x192_seed3_mi15_wpp": ((0, 0), (1, 0))}


def encode(c, args):
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "in.yuv"), "wb").write(c["input"])
        for attempt in range(6):                 # (the reference's GT search reads past its reference picture buffer; now and then that kills the process: tools/make_golden_slicedata.py)
            r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "TAppEncoderRef")] + args, cwd=td, capture_output=True, text=True)
            if r.returncode != -11: break
        assert r.returncode == 0, r.stdout[-2000:]
        return open(os.path.join(td, "s.bin"), "rb").read()


def split(data):
    """(units that must not change, the slice NAL units) of a stream; the picture-hash SEI (suffix SEI, type 40) follows the reconstruction and is left out"""
    units = U.nal_units(data)
    kind = [(u[0] >> 1) & 0x3F for u in units]
    return [(k, u) for k, u in zip(kind, units) if k >= 32 and k != 40], [u for k, u in zip(kind, units) if k < 32]


def main():
    cases = U.slice_cases()
    G = U.load_fixture()
    out = {}
    for key, modes in MODES.items():
        c = cases[key]
        assert c["frames"] == 1
        on = G[key + "/bin"].tobytes()
        fixed_on, slices_on = split(on)
        got = {}
        for rdoq, ts in modes:
            args = c["args"] + ["--RDOQ=%d" % rdoq, "--RDOQTS=%d" % ts]
            b = encode(c, args)
            name = "%s_rdoq%d%d" % (key, rdoq, ts)
            out[name + "/bin"] = np.frombuffer(b, np.uint8)
            out[name + "/args"] = np.frombuffer(" ".join(args).encode(), np.uint8)
            fixed, slices = split(b)
            assert fixed == fixed_on, "%s: a parameter set or prefix SEI changed with the switch" % name
            assert len(slices) == len(slices_on) == 1 and slices[0] != slices_on[0], "%s: the slice does not change with the switch: take another case" % name
            got[(rdoq, ts)] = slices[0]
            print(name, len(b), "bytes (RDOQ on:", len(on), "bytes)", flush=True)
        if (1, 0) in got:
            assert got[(1, 0)] != got[(0, 0)], "%s: the mixed stream equals the RDOQ-off one: no unit without transform skip changes" % key
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
