"""The timelapse output (mis_timelapse_warp_batch) on the MI355X, on config 3's sixteen 4K cameras, spherical warper,
compose scale = the median focal, both canvas types ("crop": the frames' intersection, "as_is": their union).  Config 3 is a 225
degree sweep whose frames have no common intersection: "crop" refuses it by name (recorded), so "crop" -- and "as_is" beside it --
is measured on the same sixteen cameras with a yaw step of 1 degree in place of 15 (rig "config3_1deg": a hand-held timelapse):
  (a) the fused batch to packed 8UC3 through mis_timelapse_warp_batch_timed (HIP events around back-to-back launches);
  (b) the three-pass route it replaces -- mis_warper_warp_fused_batch to 16SC3 + mask, sixteen placements into the canvas
      (Timelapser.process), sixteen clamps to 8-bit -- in alternating windows of the same process (host clock ending in a device
      synchronise; the fused batch is measured this way too, so that the two compare like with like);
  (c) the fused kernel's bytes moved (every canvas byte written once, every source byte read once at least) against 8 TB/s, and
      the spherical fused batch warp of the same rois (mis_warp_spherical_fused_batch_timed) as the yardstick;
  (d) the whole Stitcher.compose_timelapse + imencode_batch call on a kept registration.

  python tools/timelapse_bench.py [--out profiles/timelapse_v1.json]

Protocol of tools/mercator_bench.py: 7 windows per setting, settings alternated in one process after a warm-up; median and
max - min spread.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
import mercator_bench as mb                            # noqa: E402

HBM_BYTES_PER_S = 8e12


def measure_rig(ctx, st, cams, types, a):
    size = (cams[0]["width"], cams[0]["height"])
    n = len(cams)
    scale = isa.Stitcher.warped_image_scale(cams)
    kind = isa.WARP_SPHERICAL
    frames = [synth.render_frame_gpu(c) for c in cams]
    rois = st.warp_rois(ctx, scale, size, cams, kind)
    corners, sizes = [r[:2] for r in rois], [r[2:] for r in rois]
    warper = st.RotationWarper(ctx, scale, kind)
    fused = [warper.alloc_fused(r) for r in rois]
    res = {"frames": n, "frame_size": list(size), "scale": scale, "rois": [list(r) for r in rois], "types": {}}
    src_bytes = n * size[0] * size[1] * 3
    res["spherical_fused_batch_event_us"] = warper.warp_fused_batch_timed(frames, cams, rois, [f[0] for f in fused], [f[1] for f in fused], a.event_repeats)
    res["spherical_fused_batch_bytes"] = src_bytes + sum(r[2] * r[3] * 7 for r in rois)
    for ttype in types:
        try:
            dst_roi = st.result_roi(corners, sizes) if ttype == "as_is" else st.result_roi_intersection(corners, sizes)
        except ValueError as e:
            res["types"][ttype] = {"refused": str(e)}
            continue
        x, y, w, h = dst_roi
        canv8 = [st._empty_image(ctx, h, w, 3, torch.uint8) for _ in range(n)]
        canv16 = [st._empty_image(ctx, h, w, 3, torch.int16) for _ in range(n)]
        tl = st.Timelapser(ctx, ttype)
        tl.initialize(corners, sizes)

        def fused_batch():
            st.timelapse_warp_batch(ctx, kind, frames, cams, rois, scale, dst_roi, None, True, canv8)

        def three_pass():
            outs = warper.warp_fused_batch(frames, cams, rois)
            for k, (t, img, _) in enumerate(outs):
                tl.process(img, None, t, dst=canv16[k])
                torch.clamp(canv16[k], 0, 255, out=canv16[k])
                canv8[k].copy_(canv16[k])

        t = mb.alternate({"fused_batch_u8": fused_batch, "three_pass": three_pass}, a.iters, a.repeats)
        ev = st.timelapse_warp_batch_timed(ctx, kind, frames, cams, rois, scale, dst_roi, None, canv8, True, a.event_repeats)
        # bytes: the canvases written once; of the sources at least the part the canvases map (all of it for as_is)
        inside = sum(max(0, min(r[0] + r[2], x + w) - max(r[0], x)) * max(0, min(r[1] + r[3], y + h) - max(r[1], y)) for r in rois)
        read_bytes = int(src_bytes * inside / sum(r[2] * r[3] for r in rois))
        moved = n * w * h * 3 + read_bytes
        s = {k: mb.summary(v) for k, v in t.items()}
        res["types"][ttype] = {"dst_roi": list(dst_roi), "canvas_megapixels": n * w * h / 1e6, "mapped_megapixels": inside / 1e6, "settings": s,
                               "fused_batch_event_us": ev, "bytes_moved": moved, "us_at_8_TB_per_s": moved / HBM_BYTES_PER_S * 1e6,
                               "fraction_of_8_TB_per_s": moved / HBM_BYTES_PER_S * 1e6 / ev, "fused_vs_three_pass": s["fused_batch_u8"]["median_ms"] / s["three_pass"]["median_ms"],
                               "fused_vs_spherical_fused_batch": ev / res["spherical_fused_batch_event_us"]}
        del canv16
        # the whole call on a kept registration: compose_timelapse + imencode_batch
        sti = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(timelapse_type=ttype))
        sti.cameras, sti.indices = cams, list(range(n))

        def whole():
            canvases, _ = sti.compose_timelapse(frames)
            return st.imencode_batch(ctx, canvases)

        files = whole()
        res["types"][ttype]["compose_timelapse_imencode_batch"] = mb.summary(mb.alternate({"whole": whole}, 2, a.repeats, warmup=1)["whole"])
        res["types"][ttype]["jpeg_bytes"] = sum(len(f) for f in files)
        print(len(cams), ttype, json.dumps({k: (v["median_ms"], v["spread_ms"]) for k, v in s.items()}), "event_us", ev, flush=True)
    print(json.dumps({"spherical_fused_batch_event_us": res["spherical_fused_batch_event_us"]}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timelapse_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--event-repeats", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    st = isa.stitching
    ctx = isa.Context(0)
    base = synth.workload(a.workload)
    w0, h0 = base[0]["width"], base[0]["height"]
    near = [synth.make_camera(w0, h0, 60.0, 1.0 * i - 7.5, 0.5 * synth._gauss(i, 11), 0.5 * synth._gauss(i, 13), c["gain"]) for i, c in enumerate(base)]
    res = {"what": __doc__.split("\n\n")[0], "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one "
           "process after a warm-up; *_event_us: HIP events around %d back-to-back passes" % (a.iters, a.repeats, a.event_repeats), "workload": a.workload, "rigs": {}}
    for rig, cams, types in ((a.workload, base, ("crop", "as_is")), (a.workload + "_1deg", near, ("crop", "as_is"))):
        res["rigs"][rig] = measure_rig(ctx, st, cams, types, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
