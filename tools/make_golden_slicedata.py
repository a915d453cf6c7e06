#!/usr/bin/env python3
"""tools/make_golden_slicedata.py -- tests/golden/slice_data.npz: the bitstreams the UNMODIFIED reference encoder (oracle/_ref/TAppEncoderRef, built by build() where the
reference tree is present) writes for the slice-data cases of tests/slicedata_util.py: every picture of hoputil.PIC_CASES (tied by md5 to encoder_hop_pic.json /
encoder_hop_pic_mi15.json), the sharp 64x64 frame (intra NxN, transform skip), two wavefront pictures one and two CTUs wide, and three pictures coded without SAO.

Per case "<key>/bin" (the .bin, uint8) and "<key>/args" (the options).  Per configuration "header/<config>": the byte length of the first picture's slice header, i.e.
payload minus slice data, the slice data being what hop_slice_data_write_host writes for the picture coded by the CPU spine, deblocked and SAO-decided on the CPU (the path
oracle/enc_shim_pic.cpp takes); it must be the same for every one-substream case of the configuration (a wavefront picture's header holds its entry points).

Run in the build container, after build().  --reuse keeps the bitstreams of an existing fixture (they are checked again) and only recomputes the header lengths."""
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slicedata_util as U  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_hop_pic.json")))
GOLD.update(json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_hop_pic_mi15.json"))))


def encode(c):
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "in.yuv"), "wb").write(c["input"])
        for attempt in range(6):                 # the reference's GT search reads past its reference picture buffer; now and then that kills the process (SIGSEGV in xPatternSearchGT)
            r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "TAppEncoderRef")] + c["args"], cwd=td, capture_output=True, text=True)
            if r.returncode != -11: break
        assert r.returncode == 0, r.stdout[-2000:]
        return open(os.path.join(td, "s.bin"), "rb").read()


def main():
    cases = U.slice_cases()
    old = np.load(U.FIXTURE) if "--reuse" in sys.argv and os.path.exists(U.FIXTURE) else None
    out = {}
    for key, c in cases.items():
        b = old[key + "/bin"].tobytes() if old is not None and key + "/bin" in old.files else encode(c)
        if key in GOLD:
            assert hashlib.md5(c["input"]).hexdigest() == GOLD[key]["input_md5"] and hashlib.md5(b).hexdigest() == GOLD[key]["bin_md5"] and len(b) == GOLD[key]["bin_bytes"], key
        assert len(U.slice_payloads(b)) == c["frames"], key
        out[key + "/bin"] = np.frombuffer(b, np.uint8)
        out[key + "/args"] = np.frombuffer(" ".join(c["args"]).encode(), np.uint8)
        print(key, len(b), "bytes", flush=True)
    if "--bins-only" not in sys.argv:
        import slicedata_cpu as C
        header = {}
        for key, c in cases.items():
            if c["rows"] != 1 or not C.cpu_affordable(c):
                continue
            data, sizes = C.host_slice_data(c, 0)
            payload = U.slice_payloads(out[key + "/bin"].tobytes())[0]
            assert payload.endswith(data), key
            header.setdefault(c["config"], {})[key] = len(payload) - len(data)
            print(key, c["config"], "header", len(payload) - len(data), "slice data", len(data), flush=True)
        for cfg, h in header.items():
            assert len(set(h.values())) == 1, (cfg, h)
            out["header/" + cfg] = np.array([next(iter(h.values()))], np.int32)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
