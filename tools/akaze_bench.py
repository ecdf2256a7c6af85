"""AkazeFeatureFinder on the MI355X: what it costs, recorded as it is (no time is required of it yet).

  python tools/akaze_bench.py [--out profiles/akaze_v1.json]

What is measured, on config 3's sixteen 4K synthetic frames: one 4K detect and the batch of sixteen (host clock, the calls return
synchronised), in alternation with SiftFeatureFinder's batch on the same frames in the same process as the yardstick, 5 windows
each after a warm-up, median and max - min; the all-pairs matcher call on the sixteen AKAZE feature sets (61-byte rows: the wide
Hamming 2-NN) at the observed counts; and, from ONE `rocprofv3 --kernel-trace --stats` run of this script's child mode (detects of
frame 0 and one matcher call), every kernel's launches and time per detect, with the bytes the stencil kernels have to move
(computed from the level sizes) over their time against 8 TB/s."""
import argparse
import csv
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch         # noqa: E402

import image_stitching_amd as isa       # noqa: E402
import synth                            # noqa: E402

PEAK_TBS = 8.0


def frames_of(workload):
    return [synth.render_frame_gpu(c) for c in synth.workload(workload)]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


def stencil_bytes(w, h):
    """bytes a detect's stencil kernels have to move, by kernel: every plane read or written once per launch (float32)"""
    import refimpl_akaze as ra
    levels = ra.plan(w, h)
    out = {"akz_start_kernel": 0, "akz_flow_kernel": 0, "akz_fed_kernel": 0, "akz_deriv1_kernel": 0, "akz_deriv2_kernel": 0}
    for i, lv in enumerate(levels):
        px = lv["w"] * lv["h"]
        src = 3 * px if i == 0 else 4 * levels[i - 1]["w"] * levels[i - 1]["h"]
        out["akz_start_kernel"] += src + 8 * px
        out["akz_flow_kernel"] += 8 * px
        out["akz_fed_kernel"] += 12 * px * (ra.level_schedule(levels, i)[0] if i else 0)
        out["akz_deriv1_kernel"] += 12 * px
        out["akz_deriv2_kernel"] += 12 * px
    return out


def child(workload, calls):
    ctx = isa.Context(0)
    frames = frames_of(workload)
    size = (frames[0].shape[1], frames[0].shape[0])
    finder = isa.AkazeFeatureFinder(ctx, size)
    for _ in range(calls):
        finder.detect(frames[0])
    feats = finder.detect_batch(frames)
    isa.BestOf2NearestMatcher(ctx, 0.65)(feats)
    torch.cuda.synchronize()


def kernel_stats(a, size):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--kernel-calls", str(a.kernel_calls)]
    detects = a.kernel_calls + 16
    nbytes = stencil_bytes(*size)
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-1500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"(\w+)(<.*>)?\s*$", row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0])
                    k = m.group(1) if m else ""
                    if k.startswith("akz_") or k == "knn2_hamming_wide_kernel":
                        e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        per = {}
        for k, e in out.items():
            if k == "knn2_hamming_wide_kernel":
                per[k] = dict(launches=e["calls"], total_us=e["total_us"], note="one matcher call: 120 pairs, both directions, in one launch")
                continue
            v = dict(launches_per_detect=e["calls"] / detects, us_per_detect=e["total_us"] / detects)
            if k in nbytes:
                v["bytes_per_detect"] = nbytes[k]
                v["tb_per_s"] = nbytes[k] / (v["us_per_detect"] * 1e-6) / 1e12
                v["share_of_8_tb_per_s"] = v["tb_per_s"] / PEAK_TBS
            per[k] = v
        akz = [v for k, v in per.items() if k.startswith("akz_")]
        return dict(detects_traced=detects, kernels=per, launches_per_detect=sum(v["launches_per_detect"] for v in akz),
                    kernel_us_per_detect=sum(v["us_per_detect"] for v in akz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "akaze_v1.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-calls", type=int, default=4)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a.workload, a.kernel_calls)
    ctx = isa.Context(0)
    frames = frames_of(a.workload)
    size = (frames[0].shape[1], frames[0].shape[0])
    akaze, sift = isa.AkazeFeatureFinder(ctx, size), isa.SiftFeatureFinder(ctx, size)
    keep = {}

    def run_akaze():
        keep["akaze"] = akaze.detect_batch(frames)

    def run_sift():
        keep["sift"] = sift.detect_batch(frames)
    versions = {"akaze_detect_one_4k": lambda: akaze.detect(frames[0]), "akaze_detect_batch_16": run_akaze, "sift_detect_batch_16": run_sift}
    for fn in versions.values():
        fn()
    t = {k: [] for k in versions}
    for _ in range(a.repeats):
        for k, fn in versions.items():
            t[k].append(window(fn, 1))
    counts = [len(f) for f in keep["akaze"]]
    matcher = isa.BestOf2NearestMatcher(ctx, 0.65)
    matcher(keep["akaze"])
    tm = [window(lambda: matcher(keep["akaze"]), 1) for _ in range(a.repeats)]
    c = akaze.debug_counts()
    res = {"what": "AkazeFeatureFinder on %s's frames (%d x %dx%d) on one MI355X; SiftFeatureFinder on the same frames in the same run as the yardstick"
                   % (a.workload, len(frames), size[0], size[1]),
           "method": "host clock around synchronised calls, %d windows per setting in alternation after a warm-up; kernels from one rocprofv3 --kernel-trace --stats run"
                     % a.repeats,
           "calls": {k: summary(v) for k, v in t.items()},
           "keypoints": {"akaze": counts, "sift": [len(f) for f in keep["sift"]]},
           "last_frame_counts": c,
           "match_all_pairs_16_akaze_sets": summary(tm)}
    del keep, akaze, sift
    torch.cuda.empty_cache()
    if not a.no_kernels:
        res["kernel_trace"] = kernel_stats(a, size)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
