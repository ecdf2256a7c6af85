"""The batched fused warp (mis_warper_warp_fused_batch) of 16 x 4K frames for one warper kind, for the per-kind table of
DESIGN.md section 4.  Run each kind under the kernel tracer:

    rocprofv3 --kernel-trace --stats -- python3 tools/warp_kinds.py --kind cylindrical

The 16 cameras (hfov 60, yaws -37.5 .. 37.5 degrees, small pitch / roll) are the same for every kind, scale = f; the rois differ
by kind, so the line printed carries the output megapixels of one pass: us per frame and us per output megapixel both follow
from the tracer's total for warp_strip_batch_kernel divided by --reps."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_stitching_amd as isa  # noqa: E402


def cameras(w, h, n=16):
    f = (w / 2.0) / math.tan(math.radians(30.0))
    out = []
    for i in range(n):
        yaw, pitch, roll = math.radians(-37.5 + 5.0 * i), math.radians(2.0 * ((i % 3) - 1)), math.radians(1.0 * ((i % 2) - 0.5))
        cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]])
        out.append({"K": K.astype(np.float32), "R": R.astype(np.float32)})
    return out, float(np.float32(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="spherical", choices=sorted(isa.stitching.WARP_KINDS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    w, h = 3840, 2160
    ctx = isa.Context(0)
    kind = isa.stitching.WARP_KINDS[a.kind]
    cams, scale = cameras(w, h)
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in cams]
    rois = isa.stitching.warp_rois(ctx, scale, (w, h), cams, kind)
    warper = isa.RotationWarper(ctx, scale, kind)
    for _ in range(a.warmup):
        warper.warp_fused_batch(frames, cams, rois)
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        warper.warp_fused_batch(frames, cams, rois)
    e1.record()
    ctx.synchronize()
    mp = sum(r[2] * r[3] for r in rois) / 1e6
    wall_us = e0.elapsed_time(e1) * 1e3 / a.reps
    print(json.dumps({"kind": a.kind, "frames": len(cams), "reps": a.reps, "out_megapixels_per_pass": round(mp, 3),
                      "rois": rois, "host_wall_us_per_pass_incl_alloc": round(wall_us, 1)}))


if __name__ == "__main__":
    main()
