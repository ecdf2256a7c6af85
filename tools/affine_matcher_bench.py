"""matcher_type = "affine" on the MI355X: the matcher call and the Python StitchJob step of config 3 (16 x 4K) with the homography
matcher and with AffineBestOf2NearestMatcher, in one process, and the kernel times of both calls.

  python tools/affine_matcher_bench.py [--out profiles/affine_matcher_v1.json]

Both matchers run on the features of one job run.  Times are host clocks around windows of calls that end in a device synchronise,
after a warm-up; the two settings alternate inside one process and the spread of the windows is reported with the medians.  The
kernel times come from ONE `rocprofv3 --kernel-trace --stats` run of this script's own child mode (--kernels-child: a few calls of
each matcher, nothing else traced with it).  Needs a GPU."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd.distributed import StitchJob  # noqa: E402

MODELS = ("homography", "affine")
AFFINE_KERNELS = ("aff_draw_kernel", "aff_score_kernel", "aff_tail_kernel")
HOMOGRAPHY_KERNELS = ("draw_kernel", "hyp_quad_kernel", "hyp_count_kernel", "scan_tail_kernel", "second_calls_kernel")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(versions, iters, repeats, warmup=3):
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


def setup(ctx, name):
    cams = synth.workload(name)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    jobs = {m: StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path(matcher_type=m)) for m in MODELS}
    return cams, frames, jobs


def kernels_child(name, calls):
    """what the rocprofv3 run traces: `calls` matcher calls of each model on one run's features"""
    ctx = isa.Context(0)
    _, frames, jobs = setup(ctx, name)
    feats = jobs["homography"].run(frames)["features"]
    for m in MODELS:
        for _ in range(calls):
            jobs[m].engine.match(feats, 0, 1)
    torch.cuda.synchronize()


def kernel_stats(name, calls):
    """-> {kernel: {calls, total_us, mean_us}} of the RANSAC kernels of both models, from one rocprofv3 run of --kernels-child"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--kernels-child", "--workload", name, "--kernel-calls", str(calls)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-1500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    # "(anonymous namespace)::aff_score_kernel(HomoCall const*, ...)" -> "aff_score_kernel"
                    k = row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1:]
                    k = k[0].split("::")[-1] if k else ""
                    if k in AFFINE_KERNELS + HOMOGRAPHY_KERNELS:
                        e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for e in out.values():
            e["mean_us"] = e["total_us"] / max(e["calls"], 1)
        out["matcher_calls_per_model"] = calls
        for label, ks in (("affine", AFFINE_KERNELS), ("homography", HOMOGRAPHY_KERNELS)):
            out["ransac_kernels_us_per_call_" + label] = sum(out[k]["total_us"] for k in ks if k in out) / calls
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_matcher_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel-calls", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.kernels_child:
        return kernels_child(a.workload, a.kernel_calls)
    ctx = isa.Context(0)
    cams, frames, jobs = setup(ctx, a.workload)
    first = {m: jobs[m].run(frames) for m in MODELS}
    feats = first["homography"]["features"]
    keep = {}

    def match(job):
        def fn():
            keep["pm"] = job.engine.match(feats, 0, 1)
        return fn
    t_match = alternate({m: match(jobs[m]) for m in MODELS}, a.iters, a.repeats)
    keep.clear()
    t_step = alternate({m: (lambda j=jobs[m]: j.run(frames)) for m in MODELS}, a.iters, a.repeats)
    res = {"what": "AffineBestOf2NearestMatcher against BestOf2NearestMatcher on one MI355X: the matcher call on one run's features and the Python StitchJob step (hot path)",
           "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one process after a warm-up" % (a.iters, a.repeats),
           "workload": a.workload, "frames": len(cams),
           "kept": {m: [int(i) for i in first[m]["indices"]] for m in MODELS},
           "matcher_call": {m: summary(v) for m, v in t_match.items()}, "step": {m: summary(v) for m, v in t_step.items()}}
    for part in ("matcher_call", "step"):
        h, f = res[part]["homography"], res[part]["affine"]
        res[part]["affine_over_homography"] = f["median_ms"] / h["median_ms"]
        res[part]["beyond_spread"] = abs(h["median_ms"] - f["median_ms"]) > max(h["spread_ms"], f["spread_ms"])
    ctx.close()
    torch.cuda.empty_cache()
    if not a.no_kernels:
        res["kernels"] = kernel_stats(a.workload, a.kernel_calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: res[k] for k in ("matcher_call", "step")}), flush=True)


if __name__ == "__main__":
    main()
