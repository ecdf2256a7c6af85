"""GraphCutSeamFinder(COST_COLOR) on the MI355X, on config 3's (16 x 4K) seam-scale images at seam_megapix = 0.1, beside dp_color:
the finder call of both, the graph-cut solver's counts (pairs, levels, grid nodes, round sets per level against the cap), and
optionally its kernels' times and the bench.py lines of this tree and the parent's.

  python tools/seam_graphcut_bench.py [--parent-tree path/to/a/built/checkout/of/the/parent] [--kernel-stats kernel_stats.csv]
                                      [--out profiles/seam_graphcut_v1.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/seam_graphcut_bench.py --profile-run      # then --kernel-stats <dir>/..._kernel_stats.csv

Finder times are host clocks around windows of calls (each call ends in a stream synchronise), after a warm-up; dp_color and the
graph-cut finder alternate inside one process, the spread of the windows (max - min) is reported with the medians, and the ratio
is reported whichever way it falls.  --profile-run: a warm-up and three graph-cut calls, nothing written -- the run to put under
the profiler, whose kernel statistics --kernel-stats then folds into the file (the gc_* rows).  --parent-tree: bench.py's default
metric runs alternately in that tree and in this one, in fresh processes before this one opens the device; the hot path does not
touch the new file, the lines must agree within +- 3 %; that tree's library also runs its own graph-cut call in the finders'
alternation, through the same argument arrays, and its masks are compared byte for byte.  Needs a GPU."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


def bench_line(tree, steps, warmup, timeout):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline", "--no-cpp-host", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("bench.py failed in %s:\n%s" % (tree, (r.stdout + r.stderr)[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench_trees(parent, windows, steps, warmup, timeout):
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    lines = {k: [] for k in trees}
    for w in range(windows):
        for k, tree in trees.items():
            lines[k].append(bench_line(tree, steps, warmup, timeout))
            print("bench.py, window %d, %s: %s" % (w, k, lines[k][-1].get("value")), flush=True)
    med = {k: statistics.median(l["value"] for l in v) for k, v in lines.items()}
    return {"lines": lines, "median_value": med, "this_over_parent": med["this"] / med["parent"], "within_3_percent": abs(med["this"] / med["parent"] - 1.0) <= 0.03}


def kernel_rows(path):
    """The gc_* rows of a rocprofv3 kernel_stats.csv."""
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            if "gc_" in r.get("Name", ""):
                name = r["Name"].split("gc_", 1)[1].split("(")[0]
                rows.append({"kernel": "gc_" + name, "calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "average_ns": float(r["AverageNs"]),
                             "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_graphcut_v1.json"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--kernel-stats", default=None, help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --profile-run")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--bench-windows", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--bench-timeout", type=int, default=300)
    a = ap.parse_args()
    trees = bench_trees(a.parent_tree, a.bench_windows, a.bench_steps, a.bench_warmup, a.bench_timeout) if a.parent_tree and not a.profile_run else None

    import torch
    import image_stitching_amd as isa
    import synth
    from image_stitching_amd import _capi as capi
    from image_stitching_amd import stitching as st
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    ctx = isa.Context(0)
    cams = synth.workload(a.workload)
    size = (cams[0]["width"], cams[0]["height"])
    cfg = isa.StitchConfig(compose_megapix=-1, seam_megapix=0.1)
    scale = isa.Stitcher.warped_image_scale(cams)
    items = [st.seam_scale_warp(ctx, cfg, size, synth.render_frame_gpu(c), c, scale) for c in cams]
    torch.cuda.synchronize()
    corners, images, masks = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    n = len(images)

    # the C arguments built once: every setting times the library call alone, through the same arrays
    work = [m.clone() for m in masks]
    cs = (capi.MisPoint * n)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners])
    im = (capi.MisImage * n)(*[st.as_image(i) for i in images])
    mk = (capi.MisImage * n)(*[st.as_image(m) for m in work])
    finders = {"dp_color": lambda: ctx.check(ctx.lib.mis_seam_dp(ctx.h, cs, im, mk, n, 0)),
               "graphcut": lambda: ctx.check(ctx.lib.mis_seam_graphcut(ctx.h, cs, im, mk, n, 0, 10000.0, 1000.0))}
    if a.parent_tree and not a.profile_run:     # the parent's graph-cut call through its own build of the library, on a context of its own over the same stream
        plib = C.CDLL(os.path.join(os.path.abspath(a.parent_tree), "image_stitching_amd", "libmistitch.so"))
        pctx = C.c_void_p()
        plib.mis_context_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        plib.mis_seam_graphcut.argtypes = [C.c_void_p, C.POINTER(capi.MisPoint), C.POINTER(capi.MisImage), C.POINTER(capi.MisImage), C.c_int, C.c_int, C.c_float, C.c_float]
        assert plib.mis_context_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(pctx)) == 0

        def parent_graphcut():
            assert plib.mis_seam_graphcut(pctx, cs, im, mk, n, 0, 10000.0, 1000.0) == 0
        finders = {"parent_graphcut": parent_graphcut, **finders}

    def call(f):
        for w, m in zip(work, masks):
            w.copy_(m)
        f()

    if a.profile_run:
        for _ in range(4):
            call(finders["graphcut"])
        torch.cuda.synchronize()
        ctx.close()
        return

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3
    for f in finders.values():
        for _ in range(3):
            call(f)
    t_find = {k: [] for k in finders}
    for _ in range(a.repeats):
        for k, f in finders.items():
            t_find[k].append(window(lambda: call(f), a.iters))
    changed, result = {}, {}
    for k, f in finders.items():
        call(f)
        changed[k] = int(sum((w != m).sum().item() for w, m in zip(work, masks)))
        result[k] = [w.clone() for w in work]
    stats = isa.GraphCutSeamFinder(ctx).stats()
    call(finders["graphcut"])
    repeat_equal = all(torch.equal(x, y) for x, y in zip(result["graphcut"], work))

    ratio = statistics.median(t_find["graphcut"]) / statistics.median(t_find["dp_color"])
    res = {"what": "GraphCutSeamFinder(COST_COLOR) (device push-relabel, csrc/seam_gc.hip) beside DpSeamFinder(COLOR) (host) on one MI355X: %s's %d seam-scale "
                   "frames (seam_megapix 0.1)" % (a.workload, n),
           "method": "host clock around %d calls (each ends in a stream synchronise), %d windows per finder, the finders alternated in one process after a warm-up; "
                     "spread = max - min over the windows" % (a.iters, a.repeats),
           "workload": a.workload, "frames": n, "seam_scale_image": [int(images[0].shape[1]), int(images[0].shape[0])],
           "find_ms": {k: summary(v) for k, v in t_find.items()},
           "graphcut_over_dp_color": ratio, "graphcut_beats_dp_color": ratio < 1.0,
           "graphcut": {"pairs": stats["pairs"], "levels": stats["levels"], "grid_nodes": stats["nodes"], "round_sets_per_level": stats["round_sets"],
                        "worst_round_sets": max(stats["round_sets"] or [0]), "round_set_cap": stats["round_set_cap"], "global_relabels": stats["relabels"],
                        "relabel_sweeps": stats["sweeps"], "second_call_gives_the_same_masks": bool(repeat_equal)},
           "mask_pixels_removed": changed}
    if "parent_graphcut" in finders:
        new, old = res["find_ms"]["graphcut"], res["find_ms"]["parent_graphcut"]
        res["graphcut_against_parent"] = {"median_difference_ms": new["median_ms"] - old["median_ms"], "parent_spread_ms": old["spread_ms"],
                                          "median_inside_parent_windows": old["min_ms"] <= new["median_ms"] <= old["max_ms"],
                                          "median_difference_within_parent_spread": abs(new["median_ms"] - old["median_ms"]) <= old["spread_ms"],
                                          "masks_equal_parent": all(torch.equal(x, y) for x, y in zip(result["graphcut"], result["parent_graphcut"]))}
    if a.kernel_stats:
        res["graphcut_kernels_rocprofv3"] = {"source": "rocprofv3 --kernel-trace --stats over --profile-run (a warm-up and three calls: 4 calls in all)", "rows": kernel_rows(a.kernel_stats)}
    if trees:
        res["bench_py"] = trees
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method", "bench_py", "graphcut_kernels_rocprofv3")}), flush=True)


if __name__ == "__main__":
    main()
