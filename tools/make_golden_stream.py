#!/usr/bin/env python3
"""tools/make_golden_stream.py -- tests/golden/stream_hash.npz: the bitstreams the UNMODIFIED reference encoder (oracle/_ref/TAppEncoderRef, built by build() where the
reference tree is present) writes for two of the slice-data cases (tests/stream_util.HASH_CASES) with --SEIDecodedPictureHash=3, the checksum, in place of =1, the MD5 of
tests/golden/slice_data.npz.  Only the .bin is kept ("<key>/bin", a few hundred bytes each), with the options ("<key>/args").

Everything but the SEI NAL unit must equal the MD5 golden of the same case: the hash method changes nothing else.

Run in the build container, after build()."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402
import stream_util as S  # noqa: E402


def encode(c, args):
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "in.yuv"), "wb").write(c["input"])
        for attempt in range(6):                 # (the reference's GT search reads past its reference picture buffer; now and then that kills the process: tools/make_golden_slicedata.py)
            r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "TAppEncoderRef")] + args, cwd=td, capture_output=True, text=True)
            if r.returncode != -11: break
        assert r.returncode == 0, r.stdout[-2000:]
        return open(os.path.join(td, "s.bin"), "rb").read()


def main():
    cases = U.slice_cases()
    md5 = U.load_fixture()
    out = {}
    for key in S.HASH_CASES:
        c = cases[key]
        assert "--SEIDecodedPictureHash=1" in c["args"]
        args = ["--SEIDecodedPictureHash=3" if a == "--SEIDecodedPictureHash=1" else a for a in c["args"]]
        b = encode(c, args)
        got, want = S.split_units(b), S.split_units(md5[key + "/bin"].tobytes())
        assert [t for _, _, t in got] == [t for _, _, t in want], key
        for (_, u, t), (_, v, _) in zip(got, want):
            assert (u != v and len(u) < len(v)) if t == 40 else u == v, (key, t)
        out[key + "/bin"] = np.frombuffer(b, np.uint8)
        out[key + "/args"] = np.frombuffer(" ".join(args).encode(), np.uint8)
        print(key, len(b), "bytes", flush=True)
    np.savez_compressed(S.HASH_FIXTURE, **out)
    print("wrote", S.HASH_FIXTURE, os.path.getsize(S.HASH_FIXTURE), "bytes")


if __name__ == "__main__":
    main()
