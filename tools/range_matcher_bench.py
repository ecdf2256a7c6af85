"""range_width on the MI355X: what the pair selection of BestOf2NearestRangeMatcher removes from a step of config 3 (16 x 4K) and
config 4 (64 x 4K) on one GPU, and the all-pairs step of this build against another build of the library (report only).

  python tools/range_matcher_bench.py [--workloads config3,config4] [--out profiles/range_matcher_v1.json]
  python tools/range_matcher_bench.py --against DIR      # DIR: a built checkout of the commit to compare with (bench.py alternated)

For each workload the job runs all-pairs first; w is the smallest width for which every pair whose confidence reaches conf_thresh
in that run has j - i < w; then the job runs with range_width = w.  The kept indices of the two runs must be equal.  Times are
host clocks around windows that end in a device synchronise, after a warm-up; the two settings alternate inside one process and
the spread of the repeats is reported with the medians.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd.distributed import StitchJob  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3       # ms per call of fn


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
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), repeats=len(v))


def smallest_width(conf, n, thresh):
    """the smallest w with j - i < w for every pair (i < j) whose confidence reaches the pruning's threshold"""
    c = np.asarray(conf, np.float64).reshape(n, n)
    far = [j - i for i in range(n) for j in range(i + 1, n) if c[i, j] >= thresh]
    return max(far) + 1 if far else 1


def workload_times(ctx, name, iters, repeats):
    cams = synth.workload(name)
    n = len(cams)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    cfg = isa.StitchConfig.hot_path()
    all_job = StitchJob(ctx, size, cams, config=cfg)
    first = all_job.run(frames)
    counts = [len(f) for f in first["features"]]
    w = smallest_width(torch.as_tensor(first["confidence"]).cpu().numpy(), n, cfg.conf_thresh)
    band_job = StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path(range_width=w))
    band = band_job.run(frames)
    kept_all, kept_band = [int(i) for i in first["indices"]], [int(i) for i in band["indices"]]
    same_pano = bool(torch.equal(first["pano"], band["pano"]) and torch.equal(first["mask"], band["mask"]))
    jobs = {"all_pairs": all_job, "range_width": band_job}
    feats = first["features"]
    keep = {}

    def match(job):
        def fn():
            keep["pm"] = job.engine.match(feats, 0, 1)       # the matcher call alone, on the first run's features
        return fn
    t_match = alternate({k: match(j) for k, j in jobs.items()}, iters, repeats)
    keep.clear()
    t_step = alternate({k: (lambda j=j: j.run(frames)) for k, j in jobs.items()}, iters, repeats)
    res = {"frames": n, "frame_size": list(size), "conf_thresh": cfg.conf_thresh, "range_width": w,
           "pairs": {"all_pairs": len(isa.selected_pairs(counts)), "range_width": len(isa.selected_pairs(counts, w))},
           "kept": {"all_pairs": kept_all, "range_width": kept_band, "equal": kept_all == kept_band},
           "panorama_and_mask_equal": same_pano,
           "matcher_call": {k: summary(v) for k, v in t_match.items()}, "step": {k: summary(v) for k, v in t_step.items()}}
    for part in ("matcher_call", "step"):
        a, b = res[part]["all_pairs"], res[part]["range_width"]
        res[part]["saved_ms"] = a["median_ms"] - b["median_ms"]
        res[part]["beyond_spread"] = a["median_ms"] - b["median_ms"] > max(a["spread_ms"], b["spread_ms"])
    if kept_all != kept_band:
        raise SystemExit("%s: range_width %d keeps %s, all pairs keep %s" % (name, w, kept_band, kept_all))
    return res


def against(other_root, steps, warmup, rounds):
    """bench.py (all pairs, config 3, one GPU) of this tree and of `other_root`, taking turns; each run a child process under a limit"""
    out = {"this": [], "other": []}
    sequence = []
    for rnd in range(rounds):
        turn = (("other", other_root), ("this", ROOT))
        for k, root in (turn if rnd % 2 == 0 else turn[::-1]):       # A B B A ...: whichever runs second sees the device the first one left
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                                "--no-cpu-baseline", "--no-cpp-host"], capture_output=True, text=True, timeout=400, cwd=root)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
            if r.returncode != 0 or not lines:
                raise SystemExit("bench.py failed in %s: %s%s" % (root, r.stdout[-2000:], r.stderr[-2000:]))
            out[k].append(json.loads(lines[-1])["ms_per_step"])
            sequence.append(k)
            print("bench.py (%s): %.3f ms per step" % (k, out[k][-1]), flush=True)
    res = {k: summary(v) for k, v in out.items()}
    res["values_ms"] = out
    res["run_order"] = sequence
    res["difference_of_medians_ms"] = res["this"]["median_ms"] - res["other"]["median_ms"]
    res["other_spread_against_itself_ms"] = res["other"]["spread_ms"]
    res["within_other_spread"] = abs(res["difference_of_medians_ms"]) <= res["other"]["spread_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config3,config4")
    ap.add_argument("--against", help="a built checkout of the commit to compare the all-pairs step with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_matcher_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--bench-rounds", type=int, default=6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    res = {"what": "BestOf2NearestRangeMatcher on one MI355X: the Python StitchJob (hot path) all-pairs and with the smallest range_width that keeps every pair above conf_thresh",
           "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one process after a warm-up" % (a.iters, a.repeats),
           "workloads": {}}
    if os.path.exists(a.out):                      # a run of one part keeps the other parts of an earlier run
        with open(a.out) as fh:
            old = json.load(fh)
        res["workloads"] = old.get("workloads", {})
        if "all_pairs_step_against_parent" in old:
            res["all_pairs_step_against_parent"] = old["all_pairs_step_against_parent"]

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    ctx = isa.Context(0)
    for name in [w for w in a.workloads.split(",") if w]:
        res["workloads"][name] = workload_times(ctx, name, a.iters, a.repeats)
        torch.cuda.empty_cache()
        write()
        print(json.dumps({name: {k: res["workloads"][name][k] for k in ("range_width", "pairs", "kept")}}), flush=True)
    if a.against:
        ctx.close()
        torch.cuda.empty_cache()
        res["all_pairs_step_against_parent"] = against(os.path.abspath(a.against), a.bench_steps, a.bench_warmup, a.bench_rounds)
        res["all_pairs_step_against_parent"]["method"] = ("bench.py --gpus 1 --steps %d --warmup %d (config 3, all pairs) of the other build and of this one, "
                                                          "taking turns (the order swapped every round), %d runs each" % (a.bench_steps, a.bench_warmup, a.bench_rounds))
        write()
        print(json.dumps({"all_pairs_step_against_parent": res["all_pairs_step_against_parent"]}), flush=True)


if __name__ == "__main__":
    main()
