"""The device cropper (mis_crop_rect) on the MI355X, on config 3's finished panorama and result mask:
  (a) mis_crop_rect per call: host clock around calls that end in their own synchronise, the stages' times between events on the
      context's stream (mis_crop_rect_timed), the launches and doubling rounds of a call (mis_crop_stats);
  (b) the route it replaces, on the same machine: the download of the mask, mis::crop in C++ (host/cropper_tool crop_time, one
      core), the upload of the cropped 8UC3 panorama for the JPEG encoder;
  (c) the bytes the kernels must move at least (computed from the shapes, see min_bytes) against 8 TB/s.
The two routes must agree on the rectangle, or nothing is written.

  python tools/crop_device_bench.py [--out profiles/crop_device_v1.json] [--bench-lines FILE]

--bench-lines: a file of bench.py result lines, each prefixed "parent " or "new " (taken in turns by the caller), copied into the
record.  Protocol of tools/mercator_bench.py: 7 windows per setting after a warm-up; median and max - min spread.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
import mercator_bench as mb                            # noqa: E402
from image_stitching_amd import cropper               # noqa: E402
from image_stitching_amd.distributed import StitchJob  # noqa: E402

HBM_BYTES_PER_S = 8e12
STAGES = ("mask", "label_foreground", "label_background", "border_slots_and_count_read", "successors_and_starts", "doubling_rounds",
          "count_winner_walls", "label_fill", "prefix_counts", "shrink_loop")


def min_bytes(w, h, channels, border, rounds):
    """Bytes every stage reads or writes at least once (its inputs and outputs, no neighbour re-reads, no label chasing)."""
    P, S = (w + 2) * (h + 2), 8 * border
    label = P * (1 + 4) + P * (1 + 4 + 4) + P * (4 + 4)            # init, merge, flatten
    return {"mask": w * h * channels + P, "label_foreground": label, "label_background": label, "border_slots_and_count_read": P * (1 + 4) + border * 4,
            "successors_and_starts": S * 4 + border * (4 + 8), "doubling_rounds": rounds * S * (4 + 4 + 4 + 1), "count_winner_walls": 2 * S * (1 + 4) + border * 8,
            "label_fill": label, "prefix_counts": 2 * (w * h * 4 + w * h * 4), "shrink_loop": (w + h) * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_device_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    ctx = isa.Context(0)
    cams = synth.workload(a.workload)
    size = (cams[0]["width"], cams[0]["height"])
    out = StitchJob(ctx, size, cams).run({i: synth.render_frame_gpu(c) for i, c in enumerate(cams)})
    mask = out["mask"].contiguous()
    pano8 = out["pano"].clamp(0, 255).to(torch.uint8).contiguous()
    h, w = mask.shape
    torch.cuda.synchronize()
    rect = cropper.crop_rect_device(ctx, mask)
    x, y, rw, rh = rect

    # (b) the replaced route, part by part
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "cropper_tool"])
    tool = os.path.join(ROOT, "host", "cropper_tool")
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "m.pgm"), os.path.join(tmp, "c.pgm")
        with open(src, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w, h))
            f.write(mask.cpu().numpy().tobytes())
        host_rect = tuple(int(v) for v in subprocess.check_output([tool, "crop", src, dst]).split())
        if host_rect != rect:
            raise SystemExit("the device rectangle %r is not the host cropper's %r" % (rect, host_rect))
        host_crop_ms = float(subprocess.check_output([tool, "crop_time", src, str(a.repeats)]))
    cropped_host = np.ascontiguousarray(pano8[y:y + rh, x:x + rw].cpu().numpy())

    def device_call():
        cropper.crop_rect_device(ctx, mask)

    def download():
        mask.cpu()

    def upload():
        torch.from_numpy(cropped_host).cuda()

    t = {k: mb.summary(v) for k, v in mb.alternate({"mis_crop_rect": device_call, "download_mask": download, "upload_cropped_panorama": upload}, a.iters, a.repeats).items()}

    # (a) the stages between events, and the counts of a call
    ms, r4, st = (C.c_float * 10)(), (C.c_int * 4)(), C.c_int()
    per_stage = {k: [] for k in STAGES}
    for _ in range(a.repeats + 2):
        ctx.check(ctx.lib.mis_crop_rect_timed(ctx.h, C.c_void_p(mask.data_ptr()), w, h, 1, mask.stride(0), r4, C.byref(st), ms))
        for k, v in zip(STAGES, ms):
            per_stage[k].append(v)
    stats, n = (C.c_int * 4)(), C.c_int()
    ctx.check(ctx.lib.mis_crop_stats(ctx.h, stats, 4, C.byref(n)))
    launches, rounds, border, points = stats[:]
    need = min_bytes(w, h, 1, border, rounds)
    stages = {k: {"median_ms": statistics.median(v[2:]), "min_ms": min(v[2:]), "max_ms": max(v[2:]), "min_bytes": need[k],
                  "us_at_8_TB_per_s": need[k] / HBM_BYTES_PER_S * 1e6} for k, v in per_stage.items()}
    replaced = t["download_mask"]["median_ms"] + host_crop_ms + t["upload_cropped_panorama"]["median_ms"]
    res = {"what": "mis_crop_rect on the result mask of the hot_path StitchJob against the route it replaces (mask download + mis::crop on one host core + upload of "
                   "the cropped 8UC3 panorama), one MI355X",
           "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one process after a warm-up; stage times: "
                     "HIP events between the stages of one call, median of %d calls; mis::crop: median of %d runs inside host/cropper_tool" % (a.iters, a.repeats, a.repeats, a.repeats),
           "workload": a.workload, "panorama": [w, h], "rectangle": list(rect), "launches": launches, "doubling_rounds": rounds, "border_pixels": border,
           "contour_points": points, "settings": t, "host_mis_crop_ms": host_crop_ms, "replaced_route_ms": replaced,
           "stages": stages, "stage_sum_ms": sum(s["median_ms"] for s in stages.values()), "min_bytes_total": sum(need.values()),
           "us_at_8_TB_per_s_total": sum(need.values()) / HBM_BYTES_PER_S * 1e6}
    if a.bench_lines:
        res["bench_py"] = {"parent": [], "new": []}
        for line in open(a.bench_lines):
            tag, _, js = line.partition(" ")
            if tag in res["bench_py"] and js.strip().startswith("{"):
                res["bench_py"][tag].append(json.loads(js))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("panorama", "rectangle", "launches", "doubling_rounds", "replaced_route_ms", "stage_sum_ms")}), t["mis_crop_rect"])


if __name__ == "__main__":
    main()
