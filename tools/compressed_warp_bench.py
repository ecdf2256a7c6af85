"""The compressed-plane and Panini warpers (the column-hoisted map kernels) on the MI355X, on the six cameras of config 3 whose
rois are finite under these maps (yaw -37.5 .. +37.5 degrees at hfov 60: u_ stays within +-67.5 degrees):
  (a) mis_warper_roi_batch: the full-frame scan of the four kinds against the fisheye scan;
  (b) the fused batch warp of the four kinds, each alternated with the fisheye kernel warping THE SAME rois (the warp entries take
      the roi the caller hands them, so both kernels write the same number of pixels), as microseconds per megapixel of roi, with
      the instruction-issue estimate: vector instructions per pixel (disassembly of the fused kernels, every branch counted once;
      the hoisted kernels' column part divided by the 4 rows that share it) x pixels / (256 CUs x 4 SIMDs x 32 lanes per cycle x
      2.4 GHz);
  (c) the spherical hot_path job step of this tree against the parent commit's package, each alone in a fresh process and in
      turn (tools/mercator_bench.py's solo protocol).

  python tools/compressed_warp_bench.py [--baseline-tree path/to/parent/checkout] [--out profiles/compressed_panini_warpers_v1.json]

Protocol of tools/mercator_bench.py: host clock around 10 calls ending in a device synchronise, 7 windows per setting, settings
alternated in one process after a warm-up, each on a context of its own; median and max - min spread.  Needs a GPU."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
import mercator_bench as mb                            # noqa: E402

# vector instructions per output pixel of the fused batch kernels (hipcc --cuda-device-only -S, lines starting with v_, every branch
# counted once): the hoisted kernels' row loop (label to backward branch: 1445 compressed, 1459 Panini, for a lane's 4 pixels) / 4
# plus everything in front of it (539 / 781: the frame lookup and the column terms of 4 columns) / 16 pixels of a full tile; the
# fisheye kernel by the count of DESIGN.md section 4 (1912 per lane of 4 pixels)
VALU_PER_PIXEL = {"compressedPlaneA2B1": 395, "compressedPlaneA1.5B1": 395, "paniniA2B1": 414, "paniniA1.5B1": 414, "fisheye": 478}
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
KINDS = {"compressedPlaneA2B1": isa.WARP_COMPRESSED_PLANE_A2B1, "compressedPlaneA1.5B1": isa.WARP_COMPRESSED_PLANE_A15B1,
         "paniniA2B1": isa.WARP_PANINI_A2B1, "paniniA1.5B1": isa.WARP_PANINI_A15B1}
MAX_YAW = 40.0


def warp_fn_with_rois(side, kind, rois):
    """mis_warper_warp_fused_batch of `kind` into outputs allocated once, with the rois handed over -> fn"""
    ctx, st, capi, n = side.ctx, side.st, side.capi, len(side.cams)
    warper = st.RotationWarper(ctx, side.scale, kind)
    outs = [warper.alloc_fused(r) for r in rois]
    im = (capi.MisImage * n)(*[st.as_image(side.frames[i]) for i in range(n)])
    ds = (capi.MisImage * n)(*[st.as_image(o[0]) for o in outs])
    ms = (capi.MisImage * n)(*[st.as_image(o[1]) for o in outs])
    rs = (capi.MisRect * n)(*[capi.MisRect(*[int(v) for v in r]) for r in rois])
    tls = (capi.MisPoint * n)()
    fp = C.POINTER(C.c_float)
    keep = (outs, im, ds, ms, rs, tls)

    def fn(keep=keep):
        ctx.check(ctx.lib.mis_warper_warp_fused_batch(ctx.h, kind, im, n, float(side.scale), side.Ks.ctypes.data_as(fp), side.Rs.ctypes.data_as(fp), rs, ds, ms, tls))
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressed_panini_warpers_v1.json"))
    ap.add_argument("--baseline-tree", default=None, help="a checkout of the parent commit with image_stitching_amd/libmistitch.so built")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    a = ap.parse_args()
    # (c) first: the children run before this process touches the GPU
    solo = mb.solo_processes(a) if a.baseline_tree else None
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    cams = [c for c in synth.workload(a.workload) if abs(math.degrees(math.atan2(c["R"][0][2], c["R"][2][2]))) <= MAX_YAW]
    size = (cams[0]["width"], cams[0]["height"])
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    res = {"what": "the compressed-plane and Panini warpers on one MI355X, the cameras of config 3 within +-%g degrees of yaw: (a) mis_warper_roi_batch against the "
                   "fisheye scan, (b) the fused batch warp per kind alternated with the fisheye kernel on the same rois, with the instruction-issue estimate, "
                   "(c) the spherical hot_path step against the parent commit, each alone in a fresh process" % MAX_YAW,
           "method": "host clock around %d calls (%d job steps) ending in a device synchronise, %d windows per setting, settings alternated in one process "
                     "after a warm-up" % (a.iters, a.step_iters, a.repeats),
           "workload": a.workload, "frames": len(cams), "frame_size": list(size), "source_pixels": len(cams) * size[0] * size[1],
           "lane_ops_per_s": LANE_OPS_PER_S, "valu_per_pixel": VALU_PER_PIXEL}
    # (a)
    scan_kinds = dict(KINDS, fisheye=isa.WARP_FISHEYE)
    sides = {k: mb.Side(isa, cams, frames, size) for k in scan_kinds}        # one context per setting
    v = {k: sides[k].roi_fn(kind) for k, kind in scan_kinds.items()}
    res["roi_batch"] = {k: mb.summary(t) for k, t in mb.alternate(v, a.iters, a.repeats).items()}
    for r in res["roi_batch"].values():
        r["source_megapixels_per_ms"] = res["source_pixels"] / 1e6 / r["median_ms"]
    # (b) one pair per kind: the hoisted kernel and the fisheye kernel on the same rois
    res["warp_fused_batch"] = {}
    for k, kind in KINDS.items():
        rois = sides[k].st.warp_rois(sides[k].ctx, sides[k].scale, size, cams, kind)
        mp = sum(r[2] * r[3] for r in rois) / 1e6
        pair = {k: warp_fn_with_rois(sides[k], kind, rois), "fisheye": warp_fn_with_rois(sides["fisheye"], isa.WARP_FISHEYE, rois)}
        t = {n: mb.summary(w) for n, w in mb.alternate(pair, a.iters, a.repeats).items()}
        for n, r in t.items():
            r["us_per_roi_megapixel"] = r["median_ms"] * 1e3 / mp
            r["issue_bound_ms"] = VALU_PER_PIXEL[n] * mp * 1e6 / LANE_OPS_PER_S * 1e3
            r["fraction_of_issue_bound"] = r["issue_bound_ms"] / r["median_ms"]
        res["warp_fused_batch"][k] = {"roi_megapixels": mp, "rois": [list(r) for r in rois], "hoisted": t[k], "fisheye_same_rois": t["fisheye"],
                                      "ratio_to_fisheye": t[k]["median_ms"] / t["fisheye"]["median_ms"]}
        del pair
        torch.cuda.empty_cache()
    if solo:
        res["step_solo_processes"] = {k: mb.summary(t) for k, t in solo.items()}
        res["gate_spherical_vs_parent"] = {"step_solo_processes": mb.gate(res["step_solo_processes"], "spherical", "parent_spherical")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)


if __name__ == "__main__":
    main()
