"""DpSeamFinder(COLOR_GRAD) on the MI355X, on config 3's (16 x 4K) seam-scale images at seam_megapix = 0.1: the seam finder call
with dp_color and with dp_colorgrad, the gradient kernel's time, and what the reference's own schedule -- the gradients recomputed
on the host for both images of every overlapping pair -- would have added.

  python tools/seam_colorgrad_bench.py [--parent-tree path/to/a/built/checkout/of/the/parent] [--out profiles/seam_dp_colorgrad_v1.json]

Finder times are host clocks around windows of calls (each call ends in a stream synchronise), after a warm-up; dp_color and
dp_colorgrad alternate inside one process and the spread of the windows is reported with the medians.  The kernel time is taken
between two device events around a window of mis_seam_gradients calls on device buffers (launch gaps included, no copies).  The
host figure times tests/refimpl_seam_dp_grad.gradients (numpy) on one seam-scale frame and multiplies by 2 x the number of
overlapping pairs: reported, not asserted.
The Voronoi finder's call is timed by the same host clocks in the same alternation.
--baseline-lib (default with --parent-tree: that tree's library): the parent's dp_color, dp_colorgrad and Voronoi calls alternate
with this tree's in the same windows, through the same argument arrays; every finder's masks are compared byte for byte and its
median is held to the parent's own window spread.
--parent-tree: `bench.py --pipeline reference` (dp_color inside the whole job) runs alternately in that tree and in this one, in
fresh processes before this one opens the device, then the default metric once in each; the lines go into the file with the
verdict "inside the parent's own spread".  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


def bench_line(tree, extra, timeout):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline", "--no-cpp-host"] + extra, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("bench.py failed in %s:\n%s" % (tree, (r.stdout + r.stderr)[-2000:]))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: line[k] for k in ("value", "ms_per_step", "ms_per_step_median", "ms_per_step_min", "steps", "warmup")} | {"pipeline": line["config"]["pipeline"]}


def bench_trees(parent, windows, steps, warmup, timeout):
    """-> the reference-pipeline lines of both trees, alternated, and one default line each"""
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    ref = {k: [] for k in trees}
    for w in range(windows):
        for k, tree in trees.items():
            ref[k].append(bench_line(tree, ["--pipeline", "reference", "--steps", str(steps), "--warmup", str(warmup)], timeout))
            print("bench.py --pipeline reference, window %d, %s: %.2f ms per step" % (w, k, ref[k][-1]["ms_per_step"]), flush=True)
    default = {}
    for k, tree in trees.items():
        default[k] = bench_line(tree, ["--steps", "30", "--warmup", "10"], timeout)
        print("bench.py (default metric), %s: %.1f frames/s" % (k, default[k]["value"]), flush=True)
    ms = {k: [l["ms_per_step"] for l in v] for k, v in ref.items()}
    diff = statistics.median(ms["this"]) - statistics.median(ms["parent"])
    spread = max(ms["parent"]) - min(ms["parent"])
    return {"reference_pipeline": ref, "reference_ms_per_step": {k: summary(v) for k, v in ms.items()},
            "reference_median_difference_ms": diff, "parent_spread_ms": spread, "dp_color_job_inside_parent_spread": abs(diff) <= spread,
            "default_metric": default}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_dp_colorgrad_v1.json"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--baseline-lib", default=None, help="a libmistitch.so built from the parent commit (default with --parent-tree: that tree's)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--bench-windows", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.parent_tree and not a.baseline_lib:
        a.baseline_lib = os.path.join(a.parent_tree, "image_stitching_amd", "libmistitch.so")
    trees = bench_trees(a.parent_tree, a.bench_windows, a.bench_steps, a.bench_warmup, a.bench_timeout) if a.parent_tree else None

    import numpy as np
    import torch
    import image_stitching_amd as isa
    import synth
    import refimpl_seam_dp_grad as rg
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
    overlapping = sum(1 for i in range(n) for j in range(i + 1, n)
                      if max(corners[i][0], corners[j][0]) < min(corners[i][0] + images[i].shape[1], corners[j][0] + images[j].shape[1])
                      and max(corners[i][1], corners[j][1]) < min(corners[i][1] + images[i].shape[0], corners[j][1] + images[j].shape[0]))

    # the C arguments built once: every setting times the library call alone, through the same arrays
    work = [m.clone() for m in masks]
    cs = (capi.MisPoint * n)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners])
    im = (capi.MisImage * n)(*[st.as_image(i) for i in images])
    mk = (capi.MisImage * n)(*[st.as_image(m) for m in work])
    finders = {"dp_color": lambda: ctx.check(ctx.lib.mis_seam_dp(ctx.h, cs, im, mk, n, 0)),
               "dp_colorgrad": lambda: ctx.check(ctx.lib.mis_seam_dp_colorgrad(ctx.h, cs, im, mk, n)),
               "voronoi": lambda: ctx.check(ctx.lib.mis_seam_voronoi(ctx.h, cs, mk, n))}
    if a.baseline_lib:      # the parent's finders through its own build of the library, on a context of its own over the same stream
        plib = C.CDLL(os.path.abspath(a.baseline_lib))
        pctx = C.c_void_p()
        pp, pi = C.POINTER(capi.MisPoint), C.POINTER(capi.MisImage)
        plib.mis_context_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        plib.mis_seam_dp.argtypes = [C.c_void_p, pp, pi, pi, C.c_int, C.c_int]
        plib.mis_seam_dp_colorgrad.argtypes = [C.c_void_p, pp, pi, pi, C.c_int]
        plib.mis_seam_voronoi.argtypes = [C.c_void_p, pp, pi, C.c_int]
        assert plib.mis_context_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(pctx)) == 0

        def parent_dp_color():
            assert plib.mis_seam_dp(pctx, cs, im, mk, n, 0) == 0

        def parent_dp_colorgrad():
            assert plib.mis_seam_dp_colorgrad(pctx, cs, im, mk, n) == 0

        def parent_voronoi():
            assert plib.mis_seam_voronoi(pctx, cs, mk, n) == 0
        finders = {"parent_dp_color": parent_dp_color, "parent_dp_colorgrad": parent_dp_colorgrad, "parent_voronoi": parent_voronoi, **finders}

    def call(f):
        for w, m in zip(work, masks):
            w.copy_(m)
        f()

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

    gx = [torch.empty(tuple(i.shape[:2]), dtype=torch.float32, device=i.device) for i in images]
    gy = [torch.empty_like(g) for g in gx]
    ax = (capi.MisImage * n)(*[st.as_image(g) for g in gx])
    ay = (capi.MisImage * n)(*[st.as_image(g) for g in gy])
    for _ in range(5):
        ctx.check(ctx.lib.mis_seam_gradients(ctx.h, im, n, ax, ay))
    t_kernel = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_iters):
            ctx.lib.mis_seam_gradients(ctx.h, im, n, ax, ay)
        e1.record()
        e1.synchronize()
        t_kernel.append(e0.elapsed_time(e1) / a.kernel_iters)
    px = sum(int(i.shape[0] * i.shape[1]) for i in images)
    kernel_ms = statistics.median(t_kernel)

    host_img = images[0].cpu().numpy()
    rg.gradients(host_img)
    t_host = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(10):
            rg.gradients(host_img)
        t_host.append((time.perf_counter() - t0) / 10 * 1e3)
    ok = all(np.array_equal(a_.cpu().numpy().view(np.uint32), b_.view(np.uint32)) for (a_, b_) in zip((gx[0], gy[0]), rg.gradients(host_img)))

    res = {"what": "DpSeamFinder(COLOR_GRAD) on one MI355X, %s's %d seam-scale frames (seam_megapix 0.1): the finder call per cost function, the gradient "
                   "kernel, and the host time of the reference's per-pair recomputation of the gradients" % (a.workload, n),
           "method": "finder: host clock around %d calls (each ends in a stream synchronise), %d windows per setting, settings alternated in one process after a "
                     "warm-up; kernel: device events around %d calls of mis_seam_gradients on device buffers, %d windows; host: numpy restatement of one "
                     "frame's gradients, 10 calls per window" % (a.iters, a.repeats, a.kernel_iters, a.repeats),
           "workload": a.workload, "frames": n, "seam_scale_image": [int(images[0].shape[1]), int(images[0].shape[0])], "overlapping_pairs": overlapping,
           "find_ms": {k: summary(v) for k, v in t_find.items()},
           "dp_colorgrad_minus_dp_color_ms": statistics.median(t_find["dp_colorgrad"]) - statistics.median(t_find["dp_color"]),
           "mask_pixels_removed": changed,
           "gradient_kernel": {"per_launch_ms": summary(t_kernel), "frames_per_launch": n, "pixels": px,
                               "bytes_moved": px * (3 + 8), "GB_per_s": px * (3 + 8) / (kernel_ms * 1e-3) / 1e9,
                               "equals_numpy_restatement_bit_for_bit_on_frame_0": bool(ok)},
           "host_recomputation_reported_not_asserted": {"numpy_one_frame_ms": summary(t_host), "calls_in_the_reference_schedule": 2 * overlapping,
                                                        "would_add_ms": statistics.median(t_host) * 2 * overlapping}}
    if a.baseline_lib:
        new, old = res["find_ms"]["dp_color"], res["find_ms"]["parent_dp_color"]
        res["dp_color_over_parent"] = new["median_ms"] / old["median_ms"]
        res["dp_color_slower_beyond_parent_spread"] = new["median_ms"] - old["median_ms"] > old["spread_ms"]
        res["dp_color_masks_equal_parent"] = all(torch.equal(x, y) for x, y in zip(result["dp_color"], result["parent_dp_color"]))
        # every finder against the parent's build: the median inside the parent's own window spread, the masks byte for byte
        res["against_parent"] = {k: {"median_difference_ms": res["find_ms"][k]["median_ms"] - res["find_ms"]["parent_" + k]["median_ms"],
                                     "parent_spread_ms": res["find_ms"]["parent_" + k]["spread_ms"],
                                     "median_inside_parent_windows": res["find_ms"]["parent_" + k]["min_ms"] <= res["find_ms"][k]["median_ms"] <= res["find_ms"]["parent_" + k]["max_ms"],
                                     "median_difference_within_parent_spread": abs(res["find_ms"][k]["median_ms"] - res["find_ms"]["parent_" + k]["median_ms"]) <= res["find_ms"]["parent_" + k]["spread_ms"],
                                     "masks_equal_parent": all(torch.equal(x, y) for x, y in zip(result[k], result["parent_" + k]))}
                                 for k in ("dp_color", "dp_colorgrad", "voronoi")}
    res["dp_colorgrad_masks_differ_from_dp_color"] = not all(torch.equal(x, y) for x, y in zip(result["dp_color"], result["dp_colorgrad"]))
    if trees:
        res["bench_py"] = trees
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method", "bench_py")}), flush=True)


if __name__ == "__main__":
    main()
