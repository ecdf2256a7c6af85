"""The Mercator warper on the MI355X against the spherical one, on config 3's sixteen 4K cameras:
  (a) mis_warper_roi_batch: the Mercator full-frame scan (a grid-wide reduction over 16 x 8.3 M pixels) against the spherical
      border walk;
  (b) the fused batch warp of the same frames for both kinds, as microseconds per output megapixel (the roi sizes differ);
  (c) the hot_path StitchJob step for both kinds;
  (d) the general u8 warp (mis_warper_warp, LINEAR / REFLECT, 3 channels) of one 4K frame, spherical: warp_u8_kernel carries its own
      table fill, so its code moved with the Mercator branch.

  python tools/mercator_bench.py [--baseline-tree path/to/parent/checkout] [--out profiles/mercator_v1.json]

Times are host clocks around windows of calls that end in a device synchronise, after a warm-up; the settings alternate inside one
process, each on a context of its own, and the spread of the windows is reported with the medians.  --baseline-tree names a checkout of the parent commit with
its libmistitch.so built: its package is loaded beside this tree's (under another module name, on a context of its own) and its
SPHERICAL roi call, batch warp and job step alternate with this tree's in the same windows -- the comparison that says whether the
spherical kind became slower: `slower_beyond_parent_spread` is the gate.  The step (c) is measured three ways, because in a process that
holds several jobs a job's step time depends on when it was built (measured: the job built second is the slower one from either
tree; the likely cause is the binding of streams to the process's few hardware queues in creation order): in one process with the parent's job built first, with this tree's job built first, and -- the comparison free of
that -- each tree's spherical job alone in a fresh child process of its own, parent and this tree in turn (`step_solo_processes`;
the children run before this process touches the GPU).  Needs a GPU."""
import subprocess
import argparse
import ctypes as C
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402


def load_package(tree, name):
    """image_stitching_amd of another checkout, under another module name (its relative imports stay inside it)."""
    path = os.path.join(tree, "image_stitching_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


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


def gate(res, new, old):
    n, o = res[new], res[old]
    return dict(new=new, parent=old, ratio=n["median_ms"] / o["median_ms"], slower_beyond_parent_spread=n["median_ms"] - o["median_ms"] > o["spread_ms"])


class Side:
    """One build of the package (this tree's or the parent's) with a context and the C arguments of its calls, built once."""

    def __init__(self, pkg, cams, frames, size):
        self.pkg, self.cams, self.frames, self.size = pkg, cams, frames, size
        self.st = sys.modules[pkg.__name__ + ".stitching"]
        self.capi = sys.modules[pkg.__name__ + "._capi"]
        self.ctx = pkg.Context(0)
        self.scale = pkg.Stitcher.warped_image_scale(cams)
        n = len(cams)
        self.Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cams]))
        self.Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cams]))
        self.rr = (self.capi.MisRect * n)()

    def roi_fn(self, kind):
        ctx, n = self.ctx, len(self.cams)

        def fn():
            ctx.check(ctx.lib.mis_warper_roi_batch(ctx.h, kind, float(self.scale), self.size[0], self.size[1], n,
                                                   self.Ks.ctypes.data_as(C.c_void_p), self.Rs.ctypes.data_as(C.c_void_p), self.rr))
        return fn

    def warp_fn(self, kind):
        """-> (fn, output megapixels): mis_warper_warp_fused_batch into outputs allocated once"""
        ctx, st, capi, n = self.ctx, self.st, self.capi, len(self.cams)
        rois = st.warp_rois(ctx, self.scale, self.size, self.cams, kind)
        warper = st.RotationWarper(ctx, self.scale, kind)
        outs = [warper.alloc_fused(r) for r in rois]
        im = (capi.MisImage * n)(*[st.as_image(self.frames[i]) for i in range(n)])
        ds = (capi.MisImage * n)(*[st.as_image(o[0]) for o in outs])
        ms = (capi.MisImage * n)(*[st.as_image(o[1]) for o in outs])
        rs = (capi.MisRect * n)(*[capi.MisRect(*[int(v) for v in r]) for r in rois])
        tls = (capi.MisPoint * n)()
        fp = C.POINTER(C.c_float)
        keep = (outs, im, ds, ms, rs, tls)

        def fn(keep=keep):
            ctx.check(ctx.lib.mis_warper_warp_fused_batch(ctx.h, kind, im, n, float(self.scale), self.Ks.ctypes.data_as(fp), self.Rs.ctypes.data_as(fp), rs, ds, ms, tls))
        return fn, sum(r[2] * r[3] for r in rois) / 1e6, [list(r) for r in rois]

    def warp_u8_fn(self, kind):
        """mis_warper_warp of frame 0 through the package's RotationWarper.warp (LINEAR / REFLECT, 3 channels)"""
        warper = self.st.RotationWarper(self.ctx, self.scale, kind)
        K, R = self.cams[0]["K"], self.cams[0]["R"]
        return lambda: warper.warp(self.frames[0], K, R)

    def step_fn(self, warp_type):
        dist = importlib.import_module(self.pkg.__name__ + ".distributed")
        job = dist.StitchJob(self.ctx, self.size, self.cams, config=self.st.StitchConfig.hot_path(warp_type=warp_type))
        return lambda: job.run(self.frames)


def solo_child(tree, workload, iters, repeats):
    """the spherical hot_path step of one tree alone in this process -> one JSON line with the windows"""
    pkg = isa if tree == "self" else load_package(tree, "image_stitching_amd_parent")
    cams = synth.workload(workload)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    side = Side(pkg, cams, frames, size)
    t = alternate({"spherical": side.step_fn("spherical")}, iters, repeats, warmup=3)["spherical"]
    print("SOLO " + json.dumps(t), flush=True)


def solo_processes(a, rounds=3):
    """parent and this tree in turn, `rounds` fresh processes each -> {name: windows}"""
    out = {"parent_spherical": [], "spherical": []}
    for _ in range(rounds):
        for name, tree in (("parent_spherical", a.baseline_tree), ("spherical", "self")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--solo-child", tree, "--workload", a.workload, "--step-iters", str(a.step_iters),
                                "--repeats", "5"], capture_output=True, text=True, timeout=150)
            line = [l for l in r.stdout.splitlines() if l.startswith("SOLO ")]
            if r.returncode != 0 or not line:
                raise SystemExit("solo child failed: " + (r.stdout + r.stderr)[-1500:])
            out[name] += json.loads(line[-1][5:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mercator_v1.json"))
    ap.add_argument("--baseline-tree", default=None, help="a checkout of the parent commit with image_stitching_amd/libmistitch.so built")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--solo-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.solo_child:
        return solo_child(a.solo_child, a.workload, a.step_iters, a.repeats)
    solo = solo_processes(a) if a.baseline_tree and not a.no_steps else None      # before this process initialises the GPU
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    cams = synth.workload(a.workload)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    # one context per setting: a context's block pool and scratch recycle by size, and two kinds alternating on one context would
    # measure each other's misses
    new, mer = Side(isa, cams, frames, size), Side(isa, cams, frames, size)
    old = Side(load_package(a.baseline_tree, "image_stitching_amd_parent"), cams, frames, size) if a.baseline_tree else None
    SPH, MER = isa.WARP_SPHERICAL, isa.WARP_MERCATOR
    res = {"what": "the Mercator warper against the spherical one on one MI355X, config 3's cameras: (a) mis_warper_roi_batch, (b) the fused batch warp, "
                   "(c) the hot_path StitchJob step; with --baseline-tree the parent commit's spherical calls in the same windows",
           "method": "host clock around %d calls (%d job steps) ending in a device synchronise, %d windows per setting, settings alternated in one process after a warm-up"
                     % (a.iters, a.step_iters, a.repeats),
           "workload": a.workload, "frames": len(cams), "frame_size": list(size), "source_pixels": len(cams) * size[0] * size[1]}
    # (a)
    v = {}
    if old:
        v["parent_spherical"] = old.roi_fn(SPH)
    v["spherical"], v["mercator"] = new.roi_fn(SPH), mer.roi_fn(MER)
    res["roi_batch"] = {k: summary(t) for k, t in alternate(v, a.iters, a.repeats).items()}
    res["roi_batch"]["mercator_source_megapixels_per_ms"] = res["source_pixels"] / 1e6 / res["roi_batch"]["mercator"]["median_ms"]
    # (b)
    v, mp, rois = {}, {}, {}
    if old:
        v["parent_spherical"], mp["parent_spherical"], _ = old.warp_fn(SPH)
    v["spherical"], mp["spherical"], rois["spherical"] = new.warp_fn(SPH)
    v["mercator"], mp["mercator"], rois["mercator"] = mer.warp_fn(MER)
    res["warp_fused_batch"] = {k: summary(t) for k, t in alternate(v, a.iters, a.repeats).items()}
    for k in v:
        res["warp_fused_batch"][k]["output_megapixels"] = mp[k]
        res["warp_fused_batch"][k]["us_per_output_megapixel"] = res["warp_fused_batch"][k]["median_ms"] * 1e3 / mp[k]
    res["rois"] = rois
    del v
    # (c)
    # in this process twice: the parent's job built first, then this tree's first (see the module's docstring)
    if not a.no_steps:
        for tag, first in (("step_hot_path", "parent"), ("step_hot_path_new_built_first", "new")):
            v = {}
            if old and first == "parent":
                v["parent_spherical"] = old.step_fn("spherical")
            v["spherical"] = new.step_fn("spherical")
            if old and first == "new":
                v["parent_spherical"] = old.step_fn("spherical")
            v["mercator"] = mer.step_fn("mercator")
            res[tag] = {k: summary(t) for k, t in alternate(v, a.step_iters, a.repeats, warmup=2).items()}
            del v
            if not old:
                break
    if solo:
        res["step_solo_processes"] = {k: summary(t) for k, t in solo.items()}
    # (d)
    v = {}
    if old:
        v["parent_spherical"] = old.warp_u8_fn(SPH)
    v["spherical"] = new.warp_u8_fn(SPH)
    res["warp_u8_4k"] = {k: summary(t) for k, t in alternate(v, a.iters, a.repeats).items()}
    if old:
        res["gate_spherical_vs_parent"] = {k: gate(res[k], "spherical", "parent_spherical")
                                           for k in ("roi_batch", "warp_fused_batch", "warp_u8_4k", "step_hot_path", "step_hot_path_new_built_first",
                                                     "step_solo_processes") if k in res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method", "rois")}), flush=True)


if __name__ == "__main__":
    main()
