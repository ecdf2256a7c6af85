"""The scans mode's pieces on the MI355X (report only; profiles/scans_v1.json):
  (a) warp: mis_warper_warp_fused_batch of sixteen 4K frames, kind 13 (affine) against kind 2 (plane) on the same frames, K and
      in-plane rotations -- the two kinds then have the same rois and write the same bytes, so the windows compare one instruction
      stream with the two table subtractions against the other without them;
  (b) adjuster: mis_bundle_adjust_affine_partial per call on the affine matches of sixteen 1920 x 1080 passes over one planar
      master (config 3's rotating cameras give the affine matcher no pair above conf_thresh), beside mis_bundle_adjust_ray and
      mis_bundle_adjust_reproj (mask "_____") on the same table; the two kernels' times per launch from
      ONE `rocprofv3 --kernel-trace --stats` run of this script's own child mode (--child: a few affine calls, nothing else traced);
  (c) parent comparison: bench.py's default metric for this tree and for a built checkout of the parent commit
      (--baseline-tree), three alternated child processes each.

  python tools/scans_bench.py [--baseline-tree path/to/parent/checkout] [--out profiles/scans_v1.json]

(a) and (b): host clocks around windows of calls that end in a device synchronise, after a warm-up, 7 windows per setting
alternated in one process; medians and max - min.  Needs a GPU."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd import _capi as capi          # noqa: E402
from image_stitching_amd import stitching as st        # noqa: E402

KERNELS = ("ba_eval_kernel", "ba_normal_kernel")
CONF = 0.95


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(versions, iters, repeats, warmup=2):
    for fn in versions.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            out[k].append(timed(fn, iters))
    return out


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


# ------------------------------------------------------------------------------------------------ (a) the warp
def warp_part(ctx, repeats, iters):
    w, h, n = 3840, 2160, 16
    f = 0.9 * w
    K = np.array([[f, 0, 0.5 * w], [0, f, 0.5 * h], [0, 0, 1]], np.float32)
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Rs = []
    for i in range(n):
        a = np.radians(-6.0 + 0.8 * i)
        Rs.append(np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32))
    plane, affine = isa.PlaneWarper(ctx, f), isa.AffineWarper(ctx, f)
    pc = [{"K": K, "R": R} for R in Rs]
    ac = [{"K": K, "R": np.ascontiguousarray(R.T)} for R in Rs]      # getRTfromHomogeneous makes the projector's R the transpose of H
    rois = st.warp_rois(ctx, f, (w, h), pc, isa.WARP_PLANE)
    assert rois == st.warp_rois(ctx, f, (w, h), ac, isa.WARP_AFFINE)
    a, b = plane.warp_fused_batch(frames, pc, rois), affine.warp_fused_batch(frames, ac, rois)
    ctx.synchronize()
    same = all(torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b))
    del a, b
    t = alternate({"plane": lambda: plane.warp_fused_batch(frames, pc, rois), "affine": lambda: affine.warp_fused_batch(frames, ac, rois)}, iters, repeats)
    res = {k: summary(v) for k, v in t.items()}
    mp = sum(r[2] * r[3] for r in rois) / 1e6
    return dict(frames=n, frame_size=[w, h], output_megapixels=mp, same_bytes=same, calls=res,
                affine_over_plane=res["affine"]["median_ms"] / res["plane"]["median_ms"],
                affine_outside_plane_spread=abs(res["affine"]["median_ms"] - res["plane"]["median_ms"]) > res["plane"]["spread_ms"])


# ------------------------------------------------------------------------------------------------ (b) the adjusters
def scans_frames(n=16, w=1920, h=1080, overlap=0.4):
    """n frames of w x h cut from one planar master (a wide synthetic render) at integer offsets, `overlap` of a frame shared with
    its neighbour: a scanner's passes.  Config 3 itself cannot serve: its sixteen cameras rotate, and the affine matcher keeps no
    pair of them above conf_thresh (profiles/affine_matcher_v1.json: kept [0])."""
    step = int(round(w * (1 - overlap)))
    mw, mh = step * (n - 1) + w, h + 80
    master = synth.render_frame_gpu(synth.make_camera(mw, mh, 150.0, 0.0))
    return [master[(37 * i) % 80:(37 * i) % 80 + h, step * i:step * i + w].contiguous() for i in range(n)], (w, h)


def ba_inputs(ctx, name):
    frames, size = scans_frames()
    s = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(matcher_type="affine"))
    feats = s.features(frames)
    pm = s.match(feats)
    n = len(frames)
    # the rotation adjusters beside it on the same table: pinhole cameras looking straight at the sheet
    rot = [dict(focal=2000.0, aspect=1.0, ppx=size[0] / 2, ppy=size[1] / 2, R=np.eye(3)) for _ in range(n)]
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    edges = sum(1 for i in range(n) for j in range(i + 1, n) if pm[i * n + j].confidence > CONF)
    obs = sum(int(np.count_nonzero(pm[i * n + j].inliers_mask)) for i in range(n) for j in range(i + 1, n) if pm[i * n + j].confidence > CONF)
    return arr, pm, n, st._camera_array(rot, n), st._camera_array(isa.estimate_affine_cameras(pm), n), dict(edges=edges, observations=obs), (feats, frames)


def caller(fn_of_cams, template, n):
    work = (capi.MisCameraParams * n)()

    def fn():
        C.memmove(work, template, C.sizeof(template))
        fn.rc = fn_of_cams(work)
    fn.rc = 0
    return fn


def ba_part(ctx, name, repeats, iters):
    arr, pm, n, rot, aff, counts, keep = ba_inputs(ctx, name)
    lib = ctx.lib
    versions = {"affine_partial": caller(lambda c: lib.mis_bundle_adjust_affine_partial(ctx.h, arr, pm._mis, n, CONF, c), aff, n),
                "ray": caller(lambda c: lib.mis_bundle_adjust_ray(ctx.h, arr, pm._mis, n, CONF, c), rot, n),
                "reproj": caller(lambda c: lib.mis_bundle_adjust_reproj(ctx.h, arr, pm._mis, n, CONF, b"_____", c), rot, n)}
    t = alternate(versions, iters, repeats)
    return dict(workload=name, cameras=n, **counts, calls={k: summary(v) for k, v in t.items()}, return_codes={k: fn.rc for k, fn in versions.items()})


def child(name, calls):
    ctx = isa.Context(0)
    arr, pm, n, rot, aff, counts, keep = ba_inputs(ctx, name)
    fn = caller(lambda c: ctx.lib.mis_bundle_adjust_affine_partial(ctx.h, arr, pm._mis, n, CONF, c), aff, n)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def _child_cmd(a):
    return [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--kernel-calls", str(a.kernel_calls)]


def lm_counts(a):
    r = subprocess.run(_child_cmd(a)[:-1] + ["1"], capture_output=True, text=True, timeout=600, env=dict(os.environ, MIS_BA_TRACE="1"))
    m = re.findall(r"\[ba affine\] state \d+ iters (\d+) .* evaluations (\d+) observations (\d+)", r.stderr)
    if r.returncode != 0 or not m:
        return {"error": (r.stdout + r.stderr)[-1500:]}
    it, ev, ob = m[-1]
    return dict(lm_iterations=int(it), error_evaluations=int(ev), observations=int(ob))


def kernel_stats(a):
    """-> {kernel: {calls, total_us, mean_us}} of the two kernels' affine instantiations, from one rocprofv3 run of --child"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + _child_cmd(a), capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-1500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for k in KERNELS:
                        if k in name:
                            e = out.setdefault(k, {"calls": 0, "total_us": 0.0, "name": name})
                            e["calls"] += int(row["Calls"])
                            e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for e in out.values():
            e["mean_us"] = e["total_us"] / max(e["calls"], 1)
        out["affine_calls_traced"] = a.kernel_calls
        return out


# ------------------------------------------------------------------------------------------------ (c) bench.py against the parent
def bench_part(baseline_tree, windows, steps, warmup):
    def one(tree):
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                            "--no-cpp-host"], cwd=tree, capture_output=True, text=True, timeout=900)
        for line in reversed(r.stdout.splitlines()):
            if line.startswith("{") and '"metric"' in line:
                return json.loads(line)["value"]
        raise RuntimeError((r.stdout + r.stderr)[-1500:])
    vals = {"parent": [], "this": []}
    for _ in range(windows):
        vals["parent"].append(one(baseline_tree))
        vals["this"].append(one(ROOT))
    out = {k: dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), windows=len(v)) for k, v in vals.items()}
    out["unit"] = "frames/s (bench.py --gpus 1, default workload)"
    out["within_parent_spread"] = abs(out["this"]["median"] - out["parent"]["median"]) <= out["parent"]["spread"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="scans16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scans_v1.json"))
    ap.add_argument("--baseline-tree", default=None, help="a checkout of the parent commit with its libraries built")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=2)
    ap.add_argument("--bench-windows", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a.workload, a.kernel_calls)
    res = {"what": "the scans mode's warp and adjuster on one MI355X, beside the plane warp and the ray / reprojection adjusters",
           "method": "host clock around %d calls ending in a synchronise, %d windows per setting, settings alternated in one process after a warm-up" % (a.iters, a.repeats)}
    if a.baseline_tree:     # child processes first: this process has not touched the GPU yet
        res["bench_vs_parent"] = bench_part(os.path.abspath(a.baseline_tree), a.bench_windows, a.bench_steps, a.bench_warmup)
    ctx = isa.Context(0)
    res["warp"] = warp_part(ctx, a.repeats, a.iters)
    torch.cuda.empty_cache()
    res["adjuster"] = ba_part(ctx, a.workload, a.repeats, a.iters)
    ctx.close()
    torch.cuda.empty_cache()
    res["adjuster"]["affine_call"] = lm_counts(a)
    if not a.no_kernels:
        res["adjuster"]["kernels"] = kernel_stats(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)


if __name__ == "__main__":
    main()
