"""The device cropper's algorithm on the host, without a GPU: builds tools/micro/crop_emul.cpp (the kernels of csrc/crop.hip emulated
element by element over csrc/crop_core.h) with the address and undefined-behaviour sanitizers, runs it as a program on a batch of
masks and compares every stage with image_stitching_amd/cropper.py: the external contours (first pixel and length of each), the
chosen one with its points' multiplicity, the filled mask, the rectangle or the error.  tests/test_crop_device_cpu.py runs the
same comparison on all 4 x 4 masks.

  python tools/crop_emul.py [--n 500] [--max 40] [--no-sanitize]"""
import argparse
import collections
import importlib.util
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cropper():
    """image_stitching_amd/cropper.py on its own (numpy only: the package would want the built library)"""
    spec = importlib.util.spec_from_file_location("_cropper_ref", os.path.join(ROOT, "image_stitching_amd", "cropper.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(tmp, sanitize=True):
    exe = os.path.join(tmp, "crop_emul")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, os.path.join(ROOT, "tools", "micro", "crop_emul.cpp"), "-o", exe], check=True)
    return exe


def run(exe, tmp, sources):
    """sources: uint8 arrays (H, W) or (H, W, 3) -> one dict a source with every stage's result"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(sources)))
        for s in sources:
            f.write(struct.pack("3i", s.shape[1], s.shape[0], 1 if s.ndim == 2 else 3))
            f.write(np.ascontiguousarray(s).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    out, off = [], 0
    for s in sources:
        h, w = s.shape[:2]
        head = struct.unpack_from("9i", raw, off); off += 36
        nc = head[8]
        cont = np.frombuffer(raw, np.int32, 2 * nc, off).reshape(nc, 2); off += 8 * nc
        xh = np.frombuffer(raw, np.int32, w, off); off += 4 * w
        yh = np.frombuffer(raw, np.int32, h, off); off += 4 * h
        cm = np.frombuffer(raw, np.uint8, w * h, off).reshape(h, w); off += w * h
        mult = np.frombuffer(raw, np.uint8, w * h, off).reshape(h, w); off += w * h
        out.append(dict(status=head[0], rect=tuple(head[1:5]), count=head[5], first=head[6], rounds=head[7],
                        contours=[tuple(int(v) for v in c) for c in cont], xhist=xh, yhist=yh, cmask=cm, mult=mult))
    assert off == len(raw)
    return out


def reference(crp, src):
    """The same stages from cropper.py: findExternalContours, the first contour of maximal length, fillContour, crop."""
    h, w = src.shape[:2]
    if src.ndim == 3:
        g = (src[..., 0].astype(np.int64) * 9798 + src[..., 1].astype(np.int64) * 19235 + src[..., 2].astype(np.int64) * 3735 + (1 << 14)) >> 15
    else:
        g = src
    contours = crp.findExternalContours(np.where(g > 0, 255, 0).astype(np.uint8))
    ref = dict(contours=[(c[0][1] * w + c[0][0], len(c)) for c in contours])
    if not contours:
        ref.update(status=1, count=0, first=-1)
        return ref
    best = max(range(len(contours)), key=lambda i: (len(contours[i]), -i))
    c = contours[best]
    mult = np.zeros((h, w), np.uint8)
    for (x, y), k in collections.Counter(c).items():
        mult[y, x] = k
    ref.update(count=len(c), first=c[0][1] * w + c[0][0], mult=mult, cmask=crp.fillContour(c, w, h),
               xhist=np.bincount([p[0] for p in c], minlength=w), yhist=np.bincount([p[1] for p in c], minlength=h))
    try:
        _, rect = crp.crop(src)
        ref.update(status=0, rect=tuple(int(v) for v in rect))
    except ValueError as e:
        assert "no interior rectangle" in str(e)
        ref.update(status=2)
    return ref


def differences(got, ref):
    """Names of the stages whose results differ (empty: equal)."""
    bad = [k for k in ("status", "count", "first", "contours") if got[k] != ref[k]]
    if ref["status"] != 1:
        bad += [k for k in ("mult", "cmask", "xhist", "yhist") if not np.array_equal(got[k], ref[k])]
    if ref["status"] == 0 and got["rect"] != ref["rect"]:
        bad.append("rect")
    return bad


def random_masks(n, max_side, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = rng.integers(1, max_side + 1, 2)
        out.append((rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7, 0.9])).astype(np.uint8) * 255)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--max", type=int, default=40)
    ap.add_argument("--no-sanitize", action="store_true")
    a = ap.parse_args()
    crp = cropper()
    masks = random_masks(a.n, a.max)
    with tempfile.TemporaryDirectory() as tmp:
        got = run(build(tmp, not a.no_sanitize), tmp, masks)
    bad = 0
    for m, g in zip(masks, got):
        d = differences(g, reference(crp, m))
        if d:
            bad += 1
            print("%dx%d differs in %s" % (m.shape[1], m.shape[0], ", ".join(d)))
    print("%d masks, %d differ; most doubling rounds %d" % (len(masks), bad, max(g["rounds"] for g in got)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
