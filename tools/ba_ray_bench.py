"""The ray bundle adjuster on the MI355X, on config 3's sixteen 4K cameras with 0.5 degrees of rotation noise on the start, features
and matches from the job: time per mis_bundle_adjust_ray call with its LM iterations, error evaluations and observations, the two
kernels' times per launch, and mis_bundle_adjust_reproj (mask "_____") on the same inputs from this tree and from the parent's.

  python tools/ba_ray_bench.py [--baseline-lib path/to/parent/libmistitch.so] [--out profiles/ba_ray_v1.json]

Times are host clocks around windows of calls (every call ends synchronised: the adjusters return host results), after a warm-up;
the settings alternate inside one process and the spread of the windows is reported with the medians.  --baseline-lib names a
libmistitch.so built from the parent commit: its reprojection adjuster alternates with this tree's in the same windows, which is
the comparison that says whether moving the shared host pieces into a header cost anything.  The kernel times come from ONE
`rocprofv3 --kernel-trace --stats` run of this script's own child mode (--child: a few ray calls, nothing else traced with it);
the LM counts from one more child run with MIS_BA_TRACE set.  Needs a GPU."""
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
from image_stitching_amd.distributed import StitchJob  # noqa: E402

KERNELS = ("ba_eval_kernel", "ba_normal_kernel")      # ba_eval_device.h; the child runs the ray adjuster only, so these are its instantiations
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


def inputs(ctx, name, noise_deg):
    """-> (features array, MatchesInfo table, n, template of the noisy start cameras) from one run of the job"""
    cams = synth.workload(name)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    out = StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path()).run(frames)
    feats, pm, n = out["features"], out["matches"], len(cams)
    rng = np.random.default_rng(3)
    start = [dict(focal=float(c["K"][0, 0]), aspect=float(c["K"][1, 1] / c["K"][0, 0]), ppx=float(c["K"][0, 2]), ppy=float(c["K"][1, 2]),
                  R=synth.rotation_yxz(*np.radians(rng.normal(0, noise_deg, 3))) @ c["R"]) for c in cams]
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    return arr, pm, n, st._camera_array(start, n), (feats, out)


def caller(fn_of_cams, template, n):
    """a call on a fresh copy of the start cameras (the adjusters refine in place)"""
    work = (capi.MisCameraParams * n)()

    def fn():
        C.memmove(work, template, C.sizeof(template))
        assert fn_of_cams(work) == 0
    return fn


def baseline_reproj(path, arr, pm, n):
    """the parent's reprojection adjuster, on a context of its own over the same stream and the same device keypoints"""
    lib = C.CDLL(path)
    ctx = C.c_void_p()
    lib.mis_context_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.mis_bundle_adjust_reproj.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_char_p, C.c_void_p]
    assert lib.mis_context_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    return lambda cams: lib.mis_bundle_adjust_reproj(ctx, C.addressof(arr), C.addressof(pm._mis), n, CONF, b"_____", C.addressof(cams))


def child(name, noise_deg, calls):
    ctx = isa.Context(0)
    arr, pm, n, template, keep = inputs(ctx, name, noise_deg)
    fn = caller(lambda cams: ctx.lib.mis_bundle_adjust_ray(ctx.h, arr, pm._mis, n, CONF, cams), template, n)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def _child_cmd(a, calls):
    return [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--noise-deg", str(a.noise_deg), "--kernel-calls", str(calls)]


def lm_counts(a):
    """-> iterations, error evaluations and observations of one call, from the solver's trace lines"""
    r = subprocess.run(_child_cmd(a, 1), capture_output=True, text=True, timeout=600, env=dict(os.environ, MIS_BA_TRACE="1"))
    m = re.findall(r"\[ba ray\] state \d+ iters (\d+) .* evaluations (\d+) observations (\d+)", r.stderr)
    if r.returncode != 0 or not m:
        return {"error": (r.stdout + r.stderr)[-1500:]}
    it, ev, ob = m[-1]
    return dict(lm_iterations=int(it), error_evaluations=int(ev), observations=int(ob))


def kernel_stats(a):
    """-> {kernel: {calls, total_us, mean_us}} of the two kernels, from one rocprofv3 run of --child"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + _child_cmd(a, a.kernel_calls),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-1500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"(\w+)(<.*>)?\s*$", row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0])
                    k = m.group(1) if m else ""
                    if k in KERNELS:
                        e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for e in out.values():
            e["mean_us"] = e["total_us"] / max(e["calls"], 1)
        out["ray_calls_traced"] = a.kernel_calls
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_ray_v1.json"))
    ap.add_argument("--baseline-lib", default=None, help="a libmistitch.so built from the parent commit")
    ap.add_argument("--noise-deg", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a.workload, a.noise_deg, a.kernel_calls)
    ctx = isa.Context(0)
    arr, pm, n, template, keep = inputs(ctx, a.workload, a.noise_deg)
    versions = {}
    if a.baseline_lib:      # beside this tree's reprojection adjuster in every round
        versions["parent_reproj"] = caller(baseline_reproj(a.baseline_lib, arr, pm, n), template, n)
    versions["reproj"] = caller(lambda cams: ctx.lib.mis_bundle_adjust_reproj(ctx.h, arr, pm._mis, n, CONF, b"_____", cams), template, n)
    versions["ray"] = caller(lambda cams: ctx.lib.mis_bundle_adjust_ray(ctx.h, arr, pm._mis, n, CONF, cams), template, n)
    t = alternate(versions, a.iters, a.repeats)
    res = {"what": "bundle adjustment on one MI355X: mis_bundle_adjust_ray (device evaluation) and mis_bundle_adjust_reproj with mask _____ (host evaluation) on "
                   "config 3's features and matches from the job, start cameras with %.2f degrees of rotation noise" % a.noise_deg,
           "method": "host clock around %d calls, %d windows per setting, settings alternated in one process after a warm-up" % (a.iters, a.repeats),
           "workload": a.workload, "cameras": n, "calls": {k: summary(v) for k, v in t.items()}}
    if a.baseline_lib:
        new, old = res["calls"]["reproj"], res["calls"]["parent_reproj"]
        res["reproj_over_parent"] = new["median_ms"] / old["median_ms"]
        res["reproj_slower_beyond_parent_spread"] = new["median_ms"] - old["median_ms"] > old["spread_ms"]
    del keep
    ctx.close()
    torch.cuda.empty_cache()
    res["ray_call"] = lm_counts(a)
    if "error_evaluations" in res["ray_call"]:
        res["ray_call"]["ms_per_error_evaluation"] = res["calls"]["ray"]["median_ms"] / res["ray_call"]["error_evaluations"]
        res["ray_call"]["ms_per_lm_iteration"] = res["calls"]["ray"]["median_ms"] / max(res["ray_call"]["lm_iterations"], 1)
    if not a.no_kernels:
        res["kernels"] = kernel_stats(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)


if __name__ == "__main__":
    main()
