"""The panorama mode without cameras on the MI355X, on config 3's sixteen 4K cameras, features and matches from the job: the time of
the estimator call (mis_estimate_homography_cameras, host logic); mis_bundle_adjust_ray from the ESTIMATED start beside the same
adjuster from the ground-truth-plus-0.5-degrees start of tools/ba_ray_bench.py, with LM iterations and error evaluations for
both; the estimated and the adjusted median focal against the true one; the largest adjacent-pair rotation error against the
truth before and after the adjustment.

  python tools/panorama_mode_bench.py [--out profiles/panorama_mode_v1.json]
  python tools/panorama_mode_bench.py --against DIR      # DIR: a built checkout of the parent commit (bench.py --gpus 1 alternated with this tree's)

Times are host clocks around windows of calls (every call ends synchronised: the adjusters return host results), after a warm-up;
the settings alternate inside one process and the spread of the windows is reported with the medians; the estimator is timed
over 100 calls per clock reading.  The LM counts come from one child run per start with MIS_BA_TRACE set (--child START).
--against adds tools/range_matcher_bench.py's alternation of bench.py --gpus 1 (the default metric, which runs none of this code)
between this tree and DIR, three windows each, child processes.  Nothing here is a pass / fail number.  Needs a GPU."""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
from image_stitching_amd import _capi as capi          # noqa: E402
from image_stitching_amd import stitching as st        # noqa: E402

import ba_ray_bench as rb                               # noqa: E402  (inputs, alternate, summary, caller: the ground-truth start is that tool's)

CONF = rb.CONF


def so3(R):
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
    Q = u @ vt
    return -Q if np.linalg.det(Q) < 0 else Q


def adjacent_errors(cams, truth, n):
    """Rotation error of every adjacent pair (i, i + 1) against the truth, degrees (the rotations projected on SO(3))."""
    out = []
    for i in range(n - 1):
        got = so3(np.linalg.inv(np.array(list(cams[i].R)).reshape(3, 3)) @ np.array(list(cams[i + 1].R)).reshape(3, 3))
        want = np.asarray(truth[i]["R"]).T @ np.asarray(truth[i + 1]["R"])
        out.append(math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(want.T @ got) - 1) / 2)))))
    return out


def median_focal(cams, n):
    return statistics.median(cams[i].focal for i in range(n))


def setup(ctx, workload, noise_deg):
    """-> (features array, table, n, {start name: camera template}, MisSize array, keep-alive) from one run of the job"""
    arr, pm, n, noisy, keep = rb.inputs(ctx, workload, noise_deg)
    sizes = (capi.MisSize * n)()
    for k in range(n):
        sizes[k].width, sizes[k].height = arr[k].img_w, arr[k].img_h
    est = (capi.MisCameraParams * n)()
    assert ctx.lib.mis_estimate_homography_cameras(pm._mis, n, sizes, est) == capi.MIS_OK
    return arr, pm, n, {"estimated": est, "truth_plus_noise": noisy}, sizes, keep


def ray_once(ctx, arr, pm, n, template):
    work = (capi.MisCameraParams * n)()
    C.memmove(work, template, C.sizeof(template))
    rc = ctx.lib.mis_bundle_adjust_ray(ctx.h, arr, pm._mis, n, CONF, work)
    return rc, work


def child(a):
    ctx = isa.Context(0)
    arr, pm, n, starts, sizes, keep = setup(ctx, a.workload, a.noise_deg)
    ray_once(ctx, arr, pm, n, starts[a.child])
    torch.cuda.synchronize()


def lm_counts(a, start):
    """-> iterations, error evaluations and observations of one ray call from `start`, from the solver's trace lines"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", start, "--workload", a.workload, "--noise-deg", str(a.noise_deg)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, MIS_BA_TRACE="1"))
    m = re.findall(r"\[ba ray\] state \d+ iters (\d+) .* evaluations (\d+) observations (\d+)", r.stderr)
    if r.returncode != 0 or not m:
        return {"error": (r.stdout + r.stderr)[-1500:]}
    it, ev, ob = m[-1]
    return dict(lm_iterations=int(it), error_evaluations=int(ev), observations=int(ob))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_mode_v1.json"))
    ap.add_argument("--noise-deg", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--against", default=None, help="a built checkout of the parent commit: bench.py --gpus 1 of both, alternated")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--child", default=None, choices=("estimated", "truth_plus_noise"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a)
    import synth
    truth = synth.workload(a.workload)
    ctx = isa.Context(0)
    arr, pm, n, starts, sizes, keep = setup(ctx, a.workload, a.noise_deg)
    true_f = float(truth[0]["f"])
    res = {"what": "the panorama mode without cameras on one MI355X: mis_estimate_homography_cameras on %s's match table, then mis_bundle_adjust_ray from "
                   "the estimated start beside the same adjuster from the true cameras with %.2f degrees of rotation noise" % (a.workload, a.noise_deg),
           "method": "host clock around %d calls, %d windows per setting, settings alternated in one process after a warm-up" % (a.iters, a.repeats),
           "workload": a.workload, "cameras": n, "true_focal": true_f, "starts": {}}
    usable = {}
    for name, template in starts.items():
        rc, out = ray_once(ctx, arr, pm, n, template)
        e = dict(ray_rc=rc, median_focal_start=median_focal(template, n), max_adjacent_error_deg_start=max(adjacent_errors(template, truth, n)))
        if rc == 0:
            e.update(median_focal_adjusted=median_focal(out, n), max_adjacent_error_deg_adjusted=max(adjacent_errors(out, truth, n)))
            usable[name] = template
        else:
            e["error"] = ctx.lib.mis_last_error(ctx.h).decode(errors="replace")
        e["median_focal_start_over_true"] = e["median_focal_start"] / true_f
        res["starts"][name] = e
    scratch = (capi.MisCameraParams * n)()
    versions = {"estimator_x100": lambda: [ctx.lib.mis_estimate_homography_cameras(pm._mis, n, sizes, scratch) for _ in range(100)]}
    for name, template in usable.items():
        versions["ray_from_" + name] = rb.caller(lambda cams: ctx.lib.mis_bundle_adjust_ray(ctx.h, arr, pm._mis, n, CONF, cams), template, n)
    t = rb.alternate(versions, a.iters, a.repeats)
    res["calls"] = {k: rb.summary(v) for k, v in t.items()}
    del keep
    ctx.close()
    torch.cuda.empty_cache()
    for name in usable:
        res["starts"][name]["ray_call"] = lm_counts(a, name)
    if a.against:
        import range_matcher_bench as rmb
        res["bench_against_parent"] = rmb.against(os.path.abspath(a.against), a.bench_steps, a.bench_warmup, a.bench_rounds)
        res["bench_against_parent"]["method"] = "bench.py --gpus 1 --steps %d --warmup %d of the parent build and of this one, taking turns, %d child processes each" % (
            a.bench_steps, a.bench_warmup, a.bench_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)


if __name__ == "__main__":
    main()
