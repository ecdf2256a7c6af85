"""The warpers' backward methods (mis_warper_warp_backward, _batch, mis_warper_build_maps: SURVEY A.17) on the MI355X, on config 3's
sixteen 4K cameras and the panorama they span (spherical warper, compose scale = the median focal; the panorama's content is noise:
the kernels' work does not depend on it):
  (a) the panorama (8UC3) re-projected into its sixteen cameras, (LINEAR, CONSTANT) with masks: the batch call (one grid) against
      sixteen single calls;
  (b) one 1920 x 1080 view (hfov 90) out of the panorama;
  (c) mis_warper_build_maps of a 4K frame's roi, against the time its 8 bytes per roi pixel take at 8 TB/s;
  (d) the back-warp's microseconds per output megapixel beside warp_polar_fused_batch_kernel (the fisheye fused batch warp of the
      same sixteen frames: the yardstick for an issue-bound per-pixel map), with the instructions per pixel of both, counted in the
      disassembly of the built libmistitch.so (tools/kernel_diff.py's loader: every branch counted once, per lane of 4 pixels).

  python tools/warp_backward_bench.py [--out profiles/warp_backward_v1.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o wb -- python tools/warp_backward_bench.py --once
  python tools/warp_backward_bench.py --kernel-stats <dir>/.../wb_kernel_stats.csv [--out ...]
      kernel times from a run of their own: --once runs every setting twice and writes nothing; --kernel-stats adds that trace's rows
      of the warp kernels to the profile as "kernel_trace" (no GPU needed).

Protocol of tools/mercator_bench.py: host clock around `iters` calls ending in a device synchronise, 7 windows per setting, settings
alternated in one process after a warm-up; median and max - min spread.  Needs a GPU."""
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
# the kernels the measurement compares (substrings of their mangled names: <kind, channels, mode> / <kind>)
ISA_KERNELS = {"warp_back_batch<spherical,3,linear_constant>": "warp_back_batch_kernelILi0ELi3ELi2EE",
               "warp_back_batch<fisheye,3,linear_constant>": "warp_back_batch_kernelILi4ELi3ELi2EE",
               "warp_polar_fused_batch<fisheye>": "warp_polar_fused_batch_kernelILi4EE"}


def isa_counts(lib_path):
    """instructions of the compared kernels in the built library, every branch counted once: a lane's 4 pixels and per pixel"""
    import kernel_diff
    funcs, meta = kernel_diff.load(lib_path)
    out = {}
    for label, key in ISA_KERNELS.items():
        sym = [n for n in funcs if key in n and n in meta]
        if len(sym) != 1:
            raise SystemExit("kernel %r: %d symbols in %s" % (key, len(sym), lib_path))
        ins = funcs[sym[0]]
        valu = sum(1 for i in ins if i.startswith("v_"))
        out[label] = {"symbol": sym[0], "instructions_per_lane": len(ins), "vector_alu_per_lane": valu, "instructions_per_pixel": len(ins) / 4.0,
                      "vector_alu_per_pixel": valu / 4.0, "vgprs": int(meta[sym[0]].get(".vgpr_count", -1))}
    return out


def add_kernel_stats(csv_path, out_path):
    """rows of the warp kernels from a rocprofv3 --stats kernel file -> out_path's "kernel_trace" """
    import csv
    rows = []
    with open(csv_path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            if any(k in name for k in ("warp_back", "warp_maps", "warp_polar_fused_batch", "warp_points")):
                rows.append({"kernel": name, "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                             "max_us": float(r["MaxNs"]) / 1e3, "total_us": float(r["TotalDurationNs"]) / 1e3})
    if not rows:
        raise SystemExit("%s: no warp kernel in the trace" % csv_path)
    with open(out_path) as fh:
        res = json.load(fh)
    res["kernel_trace"] = {"what": "one rocprofv3 --kernel-trace --stats run of `--once` (every setting twice, the first call of each included)", "kernels": rows}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_backward_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="every setting once after a warm-up, nothing written: the run to trace")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --once run: its warp kernels' rows are added to --out")
    a = ap.parse_args()
    if a.kernel_stats:
        return add_kernel_stats(a.kernel_stats, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    st, capi = isa.stitching, isa._capi
    cams = synth.workload(a.workload)
    size = (cams[0]["width"], cams[0]["height"])
    n = len(cams)
    ctx = isa.Context(0)
    scale = isa.Stitcher.warped_image_scale(cams)
    kind = isa.WARP_SPHERICAL
    rois = st.warp_rois(ctx, scale, size, cams, kind)
    px, py, pw, ph = st.result_roi([r[:2] for r in rois], [r[2:] for r in rois])
    pano = torch.randint(0, 256, (ph, pw, 3), dtype=torch.uint8, device=ctx.device)
    warper = st.RotationWarper(ctx, scale, kind)
    sizes = [size] * n
    views = [warper._back_view(size, 3, True) for _ in range(n)]
    ds, ms = st._images([v[0] for v in views]), st._images([v[1] for v in views])
    Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cams]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cams]))
    sz = st._c_array(capi.MisSize, (capi.MisSize(*s) for s in sizes))
    simg, tl = st.as_image(pano), capi.MisPoint(px, py)
    vp = lambda arr: arr.ctypes.data_as(__import__("ctypes").c_void_p)      # noqa: E731

    def batch():
        ctx.check(ctx.lib.mis_warper_warp_backward_batch(ctx.h, kind, simg, tl, scale, n, vp(Ks), vp(Rs), sz, capi.INTER_LINEAR, capi.BORDER_CONSTANT, ds, ms))

    def singles():
        for i in range(n):
            ctx.check(ctx.lib.mis_warper_warp_backward(ctx.h, kind, simg, tl, scale, vp(Ks[i]), vp(Rs[i]), capi.INTER_LINEAR, capi.BORDER_CONSTANT, size[0], size[1],
                                                       ds[i], ms[i]))

    hd = warper._back_view((1920, 1080), 3, True)
    hK = np.array([[960.0, 0, 960.0], [0, 960.0, 540.0], [0, 0, 1]], np.float32)      # hfov 90
    hR = np.asarray(cams[n // 2]["R"], np.float32)

    def one_hd():
        warper.warp_backward(pano, (px, py), hK, hR, (1920, 1080), with_mask=True, dst=hd[0], mask=hd[1])

    r0 = rois[0]
    xm, ym = st._empty_image(ctx, r0[3], r0[2], 1, torch.float32), st._empty_image(ctx, r0[3], r0[2], 1, torch.float32)

    def maps():
        warper.build_maps(size, cams[0]["K"], cams[0]["R"], roi=r0, xmap=xm, ymap=ym)

    # the yardstick: the fisheye fused batch warp of the same sixteen frames (warp_polar_fused_batch_kernel)
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    side = mb.Side(isa, cams, frames, size)
    polar, polar_mp, _ = side.warp_fn(isa.WARP_FISHEYE)
    fwarper = st.RotationWarper(ctx, scale, isa.WARP_FISHEYE)
    frois = st.warp_rois(ctx, scale, size, cams, isa.WARP_FISHEYE)
    fx, fy, fw, fh = st.result_roi([r[:2] for r in frois], [r[2:] for r in frois])
    fpano = torch.randint(0, 256, (min(fh, 32767), min(fw, 32767), 3), dtype=torch.uint8, device=ctx.device)
    fimg = st.as_image(fpano)

    def batch_fisheye():
        ctx.check(ctx.lib.mis_warper_warp_backward_batch(ctx.h, isa.WARP_FISHEYE, fimg, capi.MisPoint(fx, fy), scale, n, vp(Ks), vp(Rs), sz, capi.INTER_LINEAR,
                                                         capi.BORDER_CONSTANT, ds, ms))

    v = {"backward_batch_16x4k": batch, "backward_16_single_calls": singles, "backward_1920x1080": one_hd, "build_maps_4k_roi": maps,
         "polar_fused_batch_fisheye": polar, "backward_batch_16x4k_fisheye": batch_fisheye}
    if a.once:
        for fn in v.values():
            fn(); fn()
        ctx.synchronize()
        return
    t = mb.alternate(v, a.iters, a.repeats)
    res = {"what": __doc__.split("\n\n")[0], "method": "host clock around %d calls ending in a device synchronise, %d windows per setting, settings alternated in one "
           "process after a warm-up" % (a.iters, a.repeats), "workload": a.workload, "frames": n, "frame_size": list(size), "panorama": [pw, ph], "panorama_tl": [px, py],
           "fisheye_panorama": [fw, fh], "scale": scale, "settings": {k: mb.summary(x) for k, x in t.items()}}
    s = res["settings"]
    out_mp = n * size[0] * size[1] / 1e6
    for k in ("backward_batch_16x4k", "backward_16_single_calls", "backward_batch_16x4k_fisheye"):
        s[k]["output_megapixels"] = out_mp
        s[k]["us_per_output_megapixel"] = s[k]["median_ms"] * 1e3 / out_mp
    s["backward_1920x1080"]["us_per_output_megapixel"] = s["backward_1920x1080"]["median_ms"] * 1e3 / (1920 * 1080 / 1e6)
    s["polar_fused_batch_fisheye"]["output_megapixels"] = polar_mp
    s["polar_fused_batch_fisheye"]["us_per_output_megapixel"] = s["polar_fused_batch_fisheye"]["median_ms"] * 1e3 / polar_mp
    s["build_maps_4k_roi"].update(roi=list(r0), bytes=8 * r0[2] * r0[3], ms_at_8_TB_per_s=8 * r0[2] * r0[3] / HBM_BYTES_PER_S * 1e3)
    res["isa"] = isa_counts(capi.LIB_PATH)
    res["batch_vs_singles"] = s["backward_batch_16x4k"]["median_ms"] / s["backward_16_single_calls"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
        fh_.write("\n")
    print(json.dumps({k: (x["median_ms"], x["spread_ms"]) for k, x in s.items()}), flush=True)


if __name__ == "__main__":
    main()
