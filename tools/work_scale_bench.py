"""work_megapix on the MI355X: the batched work-scale resize against 16 calls of the single-image entry (the gate), the kernel's
time against its memory floor, and the feature stage / whole step of config 3 at work_megapix = 0.6 and -1 (report only).

  python tools/work_scale_bench.py --kernel-run                      # the batch alone, for `rocprofv3 --kernel-trace --stats -- ...`
  python tools/work_scale_bench.py [--kernel-stats DIR] [--out profiles/work_scale_v1.json]

Times are host clocks around windows that end in a device synchronise, after a warm-up of every shape; the two versions of a
comparison alternate inside one process and the spread of the repeats is reported with the medians.  Needs a GPU."""
import argparse
import csv
import ctypes as C
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

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd import _capi as capi          # noqa: E402
from image_stitching_amd.distributed import StitchJob  # noqa: E402
from image_stitching_amd.stitching import _empty_image, as_image  # noqa: E402

HBM_BYTES_PER_S = 8e12
WORK_MEGAPIX = 0.6


def floor_bytes(sw, sh, ws, cn=3):
    """Bytes one frame's resize has to move, from the shapes: every destination byte written once; of the source, the rows the
    destination rows tap (two each), whole -- with taps closer together than a 64-byte line every line of a tapped row is read."""
    dw, dh = int(round(sw * ws)), int(round(sh * ws))
    rows = set()
    for y in range(dh):
        v = (y + 0.5) / ws - 0.5
        y0 = min(max(int(np.floor(v)), 0), sh - 1)
        rows.update((y0, min(y0 + 1, sh - 1)))
    return dict(dst=(dw, dh), written=dw * dh * cn, source_rows=len(rows), read=len(rows) * sw * cn)


def timed(fn, sync, iters):
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e6       # us per call of fn


def alternate(versions, sync, iters, repeats):
    """versions: {name: fn}.  name -> list of `repeats` window averages (us), the versions taking turns."""
    for fn in versions.values():                          # warm-up: code objects, table cache, allocator
        for _ in range(5):
            fn()
    out = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            out[k].append(timed(fn, sync, iters))
    return out


def summary(v):
    return dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), spread_us=max(v) - min(v), repeats=len(v))


def resize_versions(ctx, frames, ws):
    n = len(frames)
    sa = (capi.MisImage * n)(*[as_image(f) for f in frames])
    dw, dh = int(round(frames[0].shape[1] * ws)), int(round(frames[0].shape[0] * ws))
    bufs_a = [_empty_image(ctx, dh, dw, 3, torch.uint8) for _ in range(n)]
    bufs_b = [_empty_image(ctx, dh, dw, 3, torch.uint8) for _ in range(n)]
    da = (capi.MisImage * n)(*[as_image(b) for b in bufs_a])
    db = (capi.MisImage * n)(*[as_image(b) for b in bufs_b])
    lib = ctx.lib

    def batch():
        ctx.check(lib.mis_resize_linear_exact_batch(ctx.h, sa, n, 0, 0, ws, ws, da))

    def singles():
        for i in range(n):
            ctx.check(lib.mis_resize_linear_exact(ctx.h, C.byref(sa[i]), 0, 0, ws, ws, C.byref(db[i])))
    return batch, singles, bufs_a, bufs_b


def kernel_stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % d)
    for r in csv.DictReader(open(files[0])):
        if "resize_batch_kernel" in r["Name"]:
            return dict(name=r["Name"], calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    raise SystemExit("resize_batch_kernel is not in %s" % files[0])


def job_times(ctx, cams, size, frames, repeats, iters):
    """Feature stage (stage_features + synchronise) and whole step (run) of the Python StitchJob at both settings, alternated."""
    jobs = {"work_megapix_0.6": StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path(work_megapix=WORK_MEGAPIX)),
            "work_megapix_-1": StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path())}
    sync = lambda: torch.cuda.synchronize()       # noqa: E731
    keep = {}

    def feat(job):
        def fn():
            keep["f"] = job.stage_features(frames)     # (the previous batch's feature blocks go back to the pool)
        return fn
    feats = alternate({k: feat(j) for k, j in jobs.items()}, sync, iters, repeats)
    keep.clear()
    steps = alternate({k: (lambda j=j: j.run(frames)) for k, j in jobs.items()}, sync, iters, repeats)
    kept = {k: j.run(frames)["indices"] for k, j in jobs.items()}
    return {k: dict(feature_stage=summary(feats[k]), step=summary(steps[k]), kept=len(kept[k])) for k in jobs}


def cpp_times(cams, tmp, steps, warmup):
    """ms per step of host/stitch_bench (mis::StitchJob) at both settings, alternated; each run a child process under a time limit."""
    exe = os.path.join(ROOT, "host", "stitch_bench")
    path = os.path.join(tmp, "work_scale_cams.txt")
    with open(path, "w") as fh:
        fh.write("%d %d %d\n" % (len(cams), cams[0]["width"], cams[0]["height"]))
        for c in cams:
            vals = [c["f"], c["K"][0, 2], c["K"][1, 2], c.get("gain", 1.0)] + [float(v) for v in np.asarray(c["R"], np.float64).reshape(9)]
            fh.write(" ".join(repr(float(v)) for v in vals) + "\n")
    out = {"work_megapix_0.6": [], "work_megapix_-1": []}
    for _ in range(3):
        for k, extra in (("work_megapix_0.6", ["--work_megapix", str(WORK_MEGAPIX)]), ("work_megapix_-1", [])):
            r = subprocess.run([exe, path, "--steps", str(steps), "--warmup", str(warmup)] + extra, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                raise SystemExit("stitch_bench failed: %s%s" % (r.stdout, r.stderr))
            out[k].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"] * 1e3)
    return {k: dict(step=summary(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-run", action="store_true", help="only launch the batch (to be run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", help="output directory of that rocprofv3 run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "work_scale_v1.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--no-cpp", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    ctx = isa.Context(0)
    cams = synth.workload("config3")
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    ws, wsize = isa.work_geometry(isa.StitchConfig.hot_path(work_megapix=WORK_MEGAPIX), size)
    flist = [frames[i] for i in range(len(cams))]
    batch, singles, bufs_a, bufs_b = resize_versions(ctx, flist, ws)
    if a.kernel_run:
        for _ in range(50):
            batch()
        torch.cuda.synchronize()
        return
    batch()
    singles()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(bufs_a, bufs_b)), "the two versions disagree"
    t = alternate({"batch_1_launch": batch, "single_16_calls": singles}, lambda: torch.cuda.synchronize(), a.iters, a.repeats)
    sb, ss = summary(t["batch_1_launch"]), summary(t["single_16_calls"])
    spread = max(sb["spread_us"], ss["spread_us"])
    fb = floor_bytes(size[0], size[1], ws)
    total = (fb["read"] + fb["written"]) * len(cams)
    floor_us = total / HBM_BYTES_PER_S * 1e6
    res = {"what": "work_megapix = %.1f on config 3 (16 x %d x %d -> %d x %d), MI355X" % (WORK_MEGAPIX, size[0], size[1], wsize[0], wsize[1]),
           "method": "host clock around %d calls ending in a device synchronise, %d windows per version, versions alternated in one process after a warm-up" % (a.iters, a.repeats),
           "gate": {"batch_1_launch": sb, "single_16_calls": ss, "run_to_run_spread_us": spread,
                    "ratio_single_over_batch": ss["median_us"] / sb["median_us"],
                    "batch_not_slower_than_singles_beyond_spread": sb["median_us"] <= ss["median_us"] + spread},
           "bytes": {"per_frame": fb, "frames": len(cams), "total": total, "floor_us_at_8TBps": floor_us}}
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        ks["share_of_floor"] = floor_us / ks["average_us"]
        ks["achieved_TBps"] = total / (ks["average_us"] * 1e-6) / 1e12
        ks["bound"] = "HBM-bound" if ks["share_of_floor"] >= 0.6 else "not HBM-bound (below 60 % of the 8 TB/s floor: issue / latency limited)"
        ks["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (--kernel-run)"
        res["kernel"] = ks
    res["python_job"] = job_times(ctx, cams, size, frames, 5, 20)
    if not a.no_cpp:
        del frames, flist, bufs_a, bufs_b
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as tmp:
            res["cpp_job"] = cpp_times(cams, tmp, 20, 5)
        res["cpp_job"]["note"] = "host/stitch_bench prints the step only; its feature stage alone is not measured"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["gate"]))
    if not res["gate"]["batch_not_slower_than_singles_beyond_spread"]:
        raise SystemExit("gate failed: the batch is slower than 16 single calls")


if __name__ == "__main__":
    main()
