"""The AKAZE finder's arithmetic on the host, without a GPU: builds tools/micro/akaze_emul.cpp (the kernels of csrc/akaze.hip
emulated element by element over csrc/akaze_core.h) with the address and undefined-behaviour sanitizers, runs it as a program on
frames and returns every stage's result in the form tests/akaze_check.py judges against tests/refimpl_akaze.py -- the same rules
as the library on the GPU (tests/test_akaze_gpu.py).  tests/test_akaze_emul_cpu.py runs it on the test shapes.

  python tools/akaze_emul.py [--no-sanitize]      the test shapes against the reference"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
PLANES = ("Lt", "Lsmooth", "flow", "Lx", "Ly", "Ldet")


def build(tmp, sanitize=True):
    exe = os.path.join(tmp, "akaze_emul")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    # (no FMA contraction: the library is built without it)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, os.path.join(ROOT, "tools", "micro", "akaze_emul.cpp"), "-o", exe], check=True)
    return exe


def run(exe, tmp, jobs):
    """jobs: (frame uint8 (H, W, 3), dict of parameters) -> one dict a job: planes (a dict a level), taus, counts, kps, class_ids, desc"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for frame, kw in jobs:
            f.write(struct.pack("5if", frame.shape[1], frame.shape[0], kw.get("n_octaves", 4), kw.get("n_octave_layers", 4), kw.get("max_points", -1),
                                kw.get("threshold", 0.001)))
            f.write(np.ascontiguousarray(frame).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    out, off = [], 0
    for _ in jobs:
        nlev, = struct.unpack_from("i", raw, off); off += 4
        planes, taus = [], []
        for _l in range(nlev):
            w, h, ns = struct.unpack_from("3i", raw, off); off += 12
            taus.append(np.frombuffer(raw, np.float32, ns, off).copy()); off += 4 * ns
            lv = {}
            for name in PLANES:
                lv[name] = np.frombuffer(raw, np.float32, w * h, off).reshape(h, w).copy(); off += 4 * w * h
            planes.append(lv)
        c = struct.unpack_from("4I", raw, off); off += 16
        nkp, = struct.unpack_from("i", raw, off); off += 4
        kps = np.frombuffer(raw, KP_DTYPE, nkp, off).copy(); off += 24 * nkp
        ids = np.frombuffer(raw, np.int32, nkp, off).copy(); off += 4 * nkp
        desc = np.frombuffer(raw, np.uint8, 61 * nkp, off).reshape(nkp, 61).copy(); off += 61 * nkp
        out.append(dict(planes=planes, taus=taus, counts=dict(candidates=c[0], suppressed=c[1], refined=c[2], kcontrast=float(np.array([c[3]], np.uint32).view(np.float32)[0])),
                        kps=kps, class_ids=ids, desc=desc))
    assert off == len(raw)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-sanitize", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import akaze_check as ac
    cases = ac.cases()
    with tempfile.TemporaryDirectory() as tmp:
        got = run(build(tmp, not a.no_sanitize), tmp, [(c["frame"], c["kw"]) for c in cases])
    for c, g in zip(cases, got):
        rep = ac.check_run(c["tag"], c["frame"], c["kw"], g)
        print(c["tag"], rep)


if __name__ == "__main__":
    main()
