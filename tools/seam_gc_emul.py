"""The graph-cut seam finder's device algorithm on the host, without a GPU: builds tools/micro/seam_gc_emul.cpp (the kernels of
csrc/seam_gc.hip emulated thread by thread over csrc/seam_gc_core.h) with the address and undefined-behaviour sanitizers, runs it on
every pair of the scenes of tests/test_refimpl_seam_graphcut_cpu.py in PairwiseSeamFinder::run order, and compares capacities,
terminals, flow value and label plane with tests/refimpl_seam_graphcut.py.  Prints the round sets, global relabels and sweeps a
pair took: what the round-set cap of seam_gc.hip is derived from can be rehearsed here before a device run.

  python tools/seam_gc_emul.py [--k 8] [--no-sanitize] [scene ...]"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_pair(exe, tmp, img1, img2, m1, m2, tl1, tl2, roi, k):
    x, y, w, h = roi
    gw, gh = w + 20, h + 20
    hdr = [m1.shape[1], m1.shape[0], m2.shape[1], m2.shape[0], x - 10 - tl1[0], y - 10 - tl1[1], x - 10 - tl2[0], y - 10 - tl2[1], gw, gh, 0, 0]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("12i2f", *hdr, 10000.0, 1000.0))
        for a in (img1, img2, m1, m2):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, fin, fout, str(k)], check=True)
    raw = open(fout, "rb").read()
    stats, flow = struct.unpack("4i", raw[:16]), struct.unpack("q", raw[16:24])[0]
    V = gw * gh
    planes = np.frombuffer(raw, np.int32, 3 * V, 24).reshape(3, gh, gw)
    lab = np.frombuffer(raw, np.uint8, V, 24 + 12 * V).reshape(gh, gw).astype(bool)
    return stats, flow, planes[0], planes[1], planes[2], lab


def main():
    import refimpl_seam_graphcut as gc
    from test_refimpl_seam_graphcut_cpu import NAMES, scene
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8, help="round sets between two global relabels (GC_K of seam_gc.hip)")
    ap.add_argument("--no-sanitize", action="store_true")
    ap.add_argument("scenes", nargs="*", default=NAMES)
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "seam_gc_emul")
        flags = ["-O2"] if a.no_sanitize else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.run(["g++", "-std=c++17", *flags, os.path.join(ROOT, "tools", "micro", "seam_gc_emul.cpp"), "-o", exe], check=True)
        for name in a.scenes:
            images, corners, masks = scene(name)
            record = {}
            want = gc.find(images, corners, masks, record=record)
            out = [np.array(m) for m in masks]
            for i, j, roi in gc.pair_list(corners, [(m.shape[1], m.shape[0]) for m in out]):
                stats, flow, cr, cd, term, lab = run_pair(exe, tmp, images[i], images[j], out[i], out[j], corners[i], corners[j], roi, a.k)
                rcr, rcd, rterm, S, value = record[(i, j)]
                ok = np.array_equal(cr, rcr) and np.array_equal(cd, rcd) and np.array_equal(term, rterm) and flow == value and np.array_equal(lab, S)
                bad += not ok
                print("%-11s pair (%d, %d) grid %3d x %3d: %s   round sets %3d, relabels %2d, sweeps %3d (at most %d a relabel)" % (
                    name, i, j, roi[2] + 20, roi[3] + 20, "equal" if ok else "DIFFERS", *stats), flush=True)
                gc.find_in_pair(images[i], images[j], out[i], out[j], corners[i], corners[j], roi)
            bad += not all(np.array_equal(x, y) for x, y in zip(out, want))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
