"""The exposure compensators on the MI355X, on config 3's (16 x 4K) seam-scale images: the feed of every type at nr_feeds 1 and 3,
the whole-frame statistics kernel's time, and the Python StitchJob step of the hot path + seam step (bench.py's
hot_path_plus_seams configuration) per type that the configuration takes.

  python tools/expos_family_bench.py [--baseline-lib path/to/parent/libmistitch.so] [--out profiles/expos_family_v1.json]

Times are host clocks around windows of calls that end in a device synchronise, after a warm-up; the settings alternate inside one
process and the spread of the windows is reported with the medians.  --baseline-lib names a libmistitch.so built from the parent
commit: its gain_blocks feed (mis_compensator_create + feed, the same seam-scale images and argument arrays) alternates with this tree's in the same
windows, which is the comparison that says whether gain_blocks with one feed became slower.  The kernel times come from ONE
`rocprofv3 --kernel-trace --stats` run of this script's own child mode (--kernels-child: a few feeds of each type, nothing else
traced with it).  Needs a GPU."""
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

import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd import _capi as capi          # noqa: E402
from image_stitching_amd import stitching as st        # noqa: E402
from image_stitching_amd.distributed import StitchJob  # noqa: E402

TYPES = ("gain", "gain_blocks", "channels", "channels_blocks")
STEP_TYPES = ("gain", "gain_blocks", "channels_blocks")      # the names the Python configuration takes ("channels": stitching.EXPOS_COMP_TYPES)
KERNELS = ("frame_stats_kernel", "overlap_stats_kernel", "unit_gain_kernel", "gain_apply_kernel")


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


def config(kind, feeds=1):
    return isa.StitchConfig(compose_megapix=-1, expos_comp_type=kind, expos_comp_nr_feeds=feeds)      # + dp_color seams: hot_path_plus_seams


def seam_images(ctx, name):
    cams = synth.workload(name)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    scale = isa.Stitcher.warped_image_scale(cams)
    items = [st.seam_scale_warp(ctx, config("gain"), size, frames[i], cams[i], scale) for i in range(len(cams))]
    torch.cuda.synchronize()
    return cams, size, frames, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]


def feed_args(corners, images, masks):
    """the C arguments of mis_compensator_feed, built once: every setting times the library call alone, through the same arrays"""
    n = len(images)
    return ((capi.MisPoint * n)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners]), (capi.MisImage * n)(*[st.as_image(i) for i in images]),
            (capi.MisImage * n)(*[st.as_image(m) for m in masks]), n)


def feeder(ctx, kind, feeds, args):
    comp = {"gain": lambda: st.GainCompensator(ctx, feeds), "channels": lambda: st.ChannelsCompensator(ctx, feeds),
            "gain_blocks": lambda: st.BlocksGainCompensator(ctx, nr_feeds=feeds), "channels_blocks": lambda: st.BlocksChannelsCompensator(ctx, nr_feeds=feeds)}[kind]()

    def fn():
        ctx.check(ctx.lib.mis_compensator_feed(comp.h, *args))
    return fn


def baseline_feeder(path, args):
    """gain_blocks' feed through another build of the library (the parent's), on a context of its own over the same stream"""
    lib = C.CDLL(path)
    ctx, comp = C.c_void_p(), C.c_void_p()
    lib.mis_context_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.mis_compensator_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.mis_compensator_feed.argtypes = [C.c_void_p, C.POINTER(capi.MisPoint), C.POINTER(capi.MisImage), C.POINTER(capi.MisImage), C.c_int]
    assert lib.mis_context_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    assert lib.mis_compensator_create(ctx, 64, 64, 2, C.byref(comp)) == 0

    def fn():
        assert lib.mis_compensator_feed(comp, *args) == 0
    return fn


def kernels_child(name, calls):
    ctx = isa.Context(0)
    _, _, _, corners, images, masks = seam_images(ctx, name)
    args = feed_args(corners, images, masks)
    for kind in TYPES:
        for feeds in (1, 3):
            fn = feeder(ctx, kind, feeds, args)
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()


def kernel_stats(name, calls):
    """-> {kernel: {calls, total_us, mean_us}} of the compensator kernels, from one rocprofv3 run of --kernels-child"""
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
                    # "void (anonymous namespace)::unit_gain_kernel<unsigned char>(unsigned char*, ...)" -> "unit_gain_kernel<unsigned char>"
                    m = re.search(r"(\w+)\s*(<[^()]*>)?\s*$", row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0])
                    k = m.group(1) + (m.group(2) or "") if m else ""
                    if k.split("<")[0] in KERNELS:
                        e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for e in out.values():
            e["mean_us"] = e["total_us"] / max(e["calls"], 1)
        out["feeds_per_type_and_nr_feeds"] = calls
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expos_family_v1.json"))
    ap.add_argument("--baseline-lib", default=None, help="a libmistitch.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.kernels_child:
        return kernels_child(a.workload, a.kernel_calls)
    ctx = isa.Context(0)
    cams, size, frames, corners, images, masks = seam_images(ctx, a.workload)
    args = feed_args(corners, images, masks)
    versions = {}
    if a.baseline_lib:      # beside this tree's gain_blocks feed in every round
        versions["parent_gain_blocks_feeds1"] = baseline_feeder(a.baseline_lib, args)
    versions.update({"%s_feeds%d" % (k, f): feeder(ctx, k, f, args) for k in ("gain_blocks", "gain", "channels", "channels_blocks") for f in (1, 3)})
    t_feed = alternate(versions, a.iters, a.repeats)
    res = {"what": "the exposure compensators on one MI355X: the feed on config 3's seam-scale images per type and nr_feeds, and the Python StitchJob step with "
                   "the seam step on (dp_color seams, full compose resolution) per type",
           "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one process after a warm-up"
                     % (a.iters, a.repeats),
           "workload": a.workload, "frames": len(cams), "seam_scale_image": [int(images[0].shape[1]), int(images[0].shape[0])],
           "feed": {k: summary(v) for k, v in t_feed.items()}}
    if a.baseline_lib:
        new, old = res["feed"]["gain_blocks_feeds1"], res["feed"]["parent_gain_blocks_feeds1"]
        res["gain_blocks_feeds1_over_parent"] = new["median_ms"] / old["median_ms"]
        res["gain_blocks_feeds1_slower_beyond_parent_spread"] = new["median_ms"] - old["median_ms"] > old["spread_ms"]
    if not a.no_steps:
        jobs = {k: StitchJob(ctx, size, cams, config=config(k)) for k in STEP_TYPES}
        t_step = alternate({k: (lambda j=jobs[k]: j.run(frames)) for k in STEP_TYPES}, a.step_iters, a.repeats, warmup=2)
        res["step_hot_path_plus_seams"] = {k: summary(v) for k, v in t_step.items()}
        del jobs
    ctx.close()
    torch.cuda.empty_cache()
    if not a.no_kernels:
        res["kernels"] = kernel_stats(a.workload, a.kernel_calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)


if __name__ == "__main__":
    main()
