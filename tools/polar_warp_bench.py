"""The fisheye and stereographic warpers (the per-pixel map kernels) on the MI355X, on config 3's sixteen 4K cameras:
  (a) mis_warper_roi_batch: the full-frame scan of both kinds against Mercator's;
  (b) the fused batch warp of both kinds against the spherical one in the same process, as microseconds per output megapixel,
      with the instruction-issue estimate of the per-pixel map: vector instructions per pixel (disassembly of
      warp_polar_fused_batch_kernel, all branches counted, divided by its 4 pixels per lane) x output pixels /
      (256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz), and the achieved fraction of it;
  (c) the spherical hot_path job step of this tree against the parent commit's package, each alone in a fresh process and in
      turn (tools/mercator_bench.py's solo protocol: the only ordering free of the build-order effect);
  (d) optionally (--polar-steps) the hot_path job step of both kinds, one job per process.

  python tools/polar_warp_bench.py [--baseline-tree path/to/parent/checkout] [--out profiles/polar_warpers_v1.json]

Protocol of tools/mercator_bench.py: host clock around 10 calls ending in a device synchronise, 7 windows per setting, settings
alternated in one process after a warm-up, each on a context of its own; median and max - min spread.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
import mercator_bench as mb                            # noqa: E402

# vector instructions per output pixel of the fused batch kernels (hipcc --cuda-device-only -S, lines starting with v_, every branch
# counted once, / 4 pixels per lane: 1912 and 2128 per lane) and of the scan kernels' loops (label to backward branch, every branch
# counted once: a wave whose lanes agree on a branch of atan / acos skips the others, so a scan can run ahead of this count); the
# spherical strip kernel is not a per-pixel map and has no entry
VALU_PER_PIXEL = {"fisheye": 478, "stereographic": 532}
SCAN_VALU_PER_PIXEL = {"mercator": 272, "fisheye": 343, "stereographic": 402}
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def polar_step_child(warp_type, workload, iters, repeats):
    """the hot_path step of one polar kind alone in this process -> one JSON line with the windows and the panorama size"""
    cams = synth.workload(workload)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    side = mb.Side(isa, cams, frames, size)
    fn = side.step_fn(warp_type)
    out = fn()
    shape = list(out["pano"].shape)
    t = mb.alternate({warp_type: fn}, iters, repeats, warmup=1)[warp_type]
    print("SOLO " + json.dumps({"windows": t, "pano_shape": shape, "kept": len(out["indices"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_warpers_v1.json"))
    ap.add_argument("--baseline-tree", default=None, help="a checkout of the parent commit with image_stitching_amd/libmistitch.so built")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--polar-steps", action="store_true", help="(d): the job step of both kinds, one fresh process each")
    ap.add_argument("--polar-step-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.polar_step_child:
        return polar_step_child(a.polar_step_child, a.workload, 1, 3)
    # (c) first: the children run before this process touches the GPU
    solo = mb.solo_processes(a) if a.baseline_tree else None
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    cams = synth.workload(a.workload)
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    kinds = {"spherical": isa.WARP_SPHERICAL, "mercator": isa.WARP_MERCATOR, "fisheye": isa.WARP_FISHEYE, "stereographic": isa.WARP_STEREOGRAPHIC}
    sides = {k: mb.Side(isa, cams, frames, size) for k in kinds}        # one context per setting
    res = {"what": "the fisheye and stereographic warpers on one MI355X, config 3's cameras: (a) mis_warper_roi_batch against Mercator's scan, (b) the fused "
                   "batch warp against the spherical one with the instruction-issue estimate, (c) the spherical hot_path step against the parent commit, "
                   "each alone in a fresh process",
           "method": "host clock around %d calls (%d job steps) ending in a device synchronise, %d windows per setting, settings alternated in one process "
                     "after a warm-up" % (a.iters, a.step_iters, a.repeats),
           "workload": a.workload, "frames": len(cams), "frame_size": list(size), "source_pixels": len(cams) * size[0] * size[1],
           "lane_ops_per_s": LANE_OPS_PER_S}
    # (a)
    v = {k: sides[k].roi_fn(kinds[k]) for k in ("mercator", "fisheye", "stereographic")}
    res["roi_batch"] = {k: mb.summary(t) for k, t in mb.alternate(v, a.iters, a.repeats).items()}
    for k, r in res["roi_batch"].items():
        r["source_megapixels_per_ms"] = res["source_pixels"] / 1e6 / r["median_ms"]
        r["valu_per_pixel"] = SCAN_VALU_PER_PIXEL[k]
        r["issue_bound_ms"] = SCAN_VALU_PER_PIXEL[k] * res["source_pixels"] / LANE_OPS_PER_S * 1e3
        r["fraction_of_issue_bound"] = r["issue_bound_ms"] / r["median_ms"]
    # (b)
    v, mp, rois = {}, {}, {}
    for k in ("spherical", "fisheye", "stereographic"):
        v[k], mp[k], rois[k] = sides[k].warp_fn(kinds[k])
    res["warp_fused_batch"] = {k: mb.summary(t) for k, t in mb.alternate(v, a.iters, a.repeats).items()}
    for k, r in res["warp_fused_batch"].items():
        r["output_megapixels"] = mp[k]
        r["us_per_output_megapixel"] = r["median_ms"] * 1e3 / mp[k]
        if k in VALU_PER_PIXEL:
            r["valu_per_pixel"] = VALU_PER_PIXEL[k]
            r["issue_bound_ms"] = VALU_PER_PIXEL[k] * mp[k] * 1e6 / LANE_OPS_PER_S * 1e3
            r["fraction_of_issue_bound"] = r["issue_bound_ms"] / r["median_ms"]
    res["rois"] = rois
    if solo:
        res["step_solo_processes"] = {k: mb.summary(t) for k, t in solo.items()}
        res["gate_spherical_vs_parent"] = {"step_solo_processes": mb.gate(res["step_solo_processes"], "spherical", "parent_spherical")}
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    write()
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method", "rois")}), flush=True)
    # (d) last, each kind's job alone in a child process (a child that runs into its time limit ends this tool: nothing is started after it)
    if a.polar_steps:
        del sides, v
        torch.cuda.empty_cache()
        res["step_hot_path_polar_solo"] = {}
        for wt in VALU_PER_PIXEL:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--polar-step-child", wt, "--workload", a.workload], capture_output=True, text=True,
                               timeout=200)
            line = [l for l in r.stdout.splitlines() if l.startswith("SOLO ")]
            if r.returncode != 0 or not line:
                raise SystemExit("polar step child failed: " + (r.stdout + r.stderr)[-1500:])
            d = json.loads(line[-1][5:])
            res["step_hot_path_polar_solo"][wt] = dict(mb.summary(d["windows"]), pano_shape=d["pano_shape"], kept=d["kept"])
            write()
        print(json.dumps(res["step_hot_path_polar_solo"]), flush=True)


if __name__ == "__main__":
    main()
