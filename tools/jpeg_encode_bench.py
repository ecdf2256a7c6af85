"""mis_jpeg_encode_batch on the MI355X: config 3's sixteen 4K synthetic frames in one batch call, and one image of config 3's
panorama size (16551 x 2167: the first frames side by side, cropped and edge-padded to that size), both at cv::imwrite's defaults
(quality 95, 4:2:0).

  python tools/jpeg_encode_bench.py [--out profiles/jpeg_encode_v1.json] [--parent DIR]

What is measured: the call (host clock; it returns synchronised) in alternation with Pillow -- libjpeg-turbo -- saving the same
pixels, the sixteen frames on sixteen host threads and the one panorama on one thread, 7 windows per setting after a warm-up, median
and max - min; the call's five parts from mis_jpeg_encode_batch_timed (the launches and the download between stream events, entropy
coding, join + stuffing and headers on the host clock); the two kernels' times from ONE `rocprofv3 --kernel-trace --stats` run of
this script's child mode, with each kernel's bytes (computed from the geometry: source pixels in, coefficients out) over that time
against 8 TB/s.  The streams are compared with Pillow's byte for byte before anything is timed.  With --parent DIR (a built checkout
of the parent commit) `bench.py --gpus 1 --steps 30 --warmup 10` runs in this tree and in that one taking turns, and the ratio of
the medians is set against the parent's own max - min.  Needs a GPU and Pillow: without Pillow there is nothing to compare with, the
tool says so and measures nothing."""
import argparse
import concurrent.futures
import csv
import ctypes as C
import glob
import io
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

import numpy as np   # noqa: E402
import torch         # noqa: E402

import image_stitching_amd as isa                      # noqa: E402
import synth                                           # noqa: E402
from image_stitching_amd import _capi as capi          # noqa: E402
from image_stitching_amd import stitching as st        # noqa: E402

KERNELS = ("jpeg_enc_luma_kernel", "jpeg_enc_chroma_kernel")
PEAK_TBS = 8.0
THREADS = 16
PANO = (16551, 2167)
QUALITY = 95
PARTS = ("launches_ms", "download_ms", "host_entropy_ms", "host_join_ms", "host_headers_ms")


def inputs(workload, which):
    """device BGR images: the workload's frames, or one image of the panorama's size made of them"""
    frames = [synth.render_frame_gpu(c) for c in synth.workload(workload)]
    if which == "frames":
        return frames
    w, h = PANO
    need = -(-w // frames[0].shape[1])
    strip = torch.cat(frames[:need], dim=1)[:, :w]
    pad = strip[-1:].expand(h - strip.shape[0], -1, -1) if h > strip.shape[0] else strip[:0]
    return [torch.cat([strip, pad], dim=0)[:h].contiguous()]


def pillow_save(rgbs, pool):
    from PIL import Image

    def one(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=QUALITY, subsampling="4:2:0", optimize=False)
        return buf.getvalue()
    return list(pool.map(one, rgbs)) if pool else [one(a) for a in rgbs]


class Encoder:
    def __init__(self, ctx, images):
        self.ctx, self.images, self.n = ctx, images, len(images)
        self.imgs = st._images(images)
        self.params = capi.MisJpegEncodeParams(QUALITY, capi.JPEG_420, 0)
        self.outs = (capi.MisJpegStream * self.n)()

    def _free(self, keep=False):
        data = [C.string_at(o.data, o.bytes) for o in self.outs] if keep else None
        for o in self.outs:
            self.ctx.lib.mis_jpeg_stream_free(C.byref(o))
        return data

    def __call__(self, keep=False):
        self.ctx.check(self.ctx.lib.mis_jpeg_encode_batch(self.ctx.h, self.imgs, self.n, C.byref(self.params), self.outs))
        return self._free(keep)

    def timed(self):
        ms = (C.c_float * 5)()
        self.ctx.check(self.ctx.lib.mis_jpeg_encode_batch_timed(self.ctx.h, self.imgs, self.n, C.byref(self.params), self.outs, ms))
        self._free()
        return list(ms)

    def kernel_bytes(self):
        """bytes each kernel has to move: the source pixels in, its coefficient planes out"""
        luma = chroma = 0
        for im in self.images:
            h, w = im.shape[:2]
            mx, my = -(-w // 16), -(-h // 16)
            luma += w * h * 3 + mx * 2 * my * 2 * 128
            chroma += w * h * 3 + 2 * mx * my * 128
        return {"jpeg_enc_luma_kernel": luma, "jpeg_enc_chroma_kernel": chroma}


def window(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) / iters * 1e3


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


def child(workload, which, calls):
    ctx = isa.Context(0)
    enc = Encoder(ctx, inputs(workload, which))
    for _ in range(calls):
        enc()
    torch.cuda.synchronize()


def kernel_stats(a, which, nbytes):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--which", which, "--kernel-calls", str(a.kernel_calls)]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-1500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"(\w+)(<.*>)?\s*$", row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0])
                    k = m.group(1) if m else ""
                    if k in KERNELS:
                        e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += float(row["TotalDurationNs"]) / 1e3
        for k, e in out.items():
            e["mean_us"] = e["total_us"] / max(e["calls"], 1)
            e["bytes"] = nbytes[k]
            e["tb_per_s"] = nbytes[k] / (e["mean_us"] * 1e-6) / 1e12
            e["share_of_8_tb_per_s"] = e["tb_per_s"] / PEAK_TBS
        out["calls_traced"] = a.kernel_calls
        return out


def bench_value(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "10"], cwd=tree, capture_output=True, text=True, timeout=900)
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and '"metric"' in line:
            return json.loads(line)["value"]
    raise SystemExit("bench.py in %s printed no result line:\n%s" % (tree, (r.stdout + r.stderr)[-1500:]))


def bench_turns(parent, rounds):
    vals = {"this_tree": [], "parent": []}
    for _ in range(rounds):
        vals["this_tree"].append(bench_value(ROOT))
        vals["parent"].append(bench_value(parent))
    med = {k: statistics.median(v) for k, v in vals.items()}
    spread = max(vals["parent"]) - min(vals["parent"])
    return {"command": "bench.py --gpus 1 --steps 30 --warmup 10, the two trees taking turns, a fresh process each", "frames_per_s": vals, "median": med,
            "ratio_this_over_parent": med["this_tree"] / med["parent"], "parent_spread_frames_per_s": spread,
            "difference_inside_parent_spread": abs(med["this_tree"] - med["parent"]) <= spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--kernel-calls", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs in both trees taking turns")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--which", default="frames", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        import PIL
        from PIL import features
    except ImportError:
        print("Pillow is not installed here: there is nothing to compare with, nothing is measured")
        return 1
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a.workload, a.which, a.kernel_calls)
    ctx = isa.Context(0)
    res = {"what": "mis_jpeg_encode_batch (quality %d, 4:2:0) of %s's frames in one call and of one %d x %d image on one MI355X against Pillow %s / "
                   "libjpeg-turbo %s saving the same pixels (the frames on %d host threads, the panorama on one)" % (QUALITY, a.workload, PANO[0], PANO[1], PIL.__version__, features.version("jpg"), THREADS),
           "method": "host clock around %d calls, %d windows per setting, the two encoders alternated in one process after a warm-up; parts from "
                     "mis_jpeg_encode_batch_timed (median of the windows' calls); kernels from one rocprofv3 --kernel-trace --stats run per input" % (a.iters, a.repeats),
           "workload": a.workload, "host_threads": min(THREADS, os.cpu_count() or 1), "inputs": {}}
    pool = concurrent.futures.ThreadPoolExecutor(THREADS)
    for which in ("frames", "panorama"):
        images = inputs(a.workload, which)
        enc = Encoder(ctx, images)
        rgbs = [np.ascontiguousarray(im.cpu().numpy()[:, :, ::-1]) for im in images]
        use_pool = pool if which == "frames" else None
        pil_name = "pillow_%d_threads" % THREADS if which == "frames" else "pillow_1_thread"
        ours, ref = enc(keep=True), pillow_save(rgbs, use_pool)
        equal = ours == ref
        nbytes_out = sum(len(d) for d in ours)
        del ours, ref
        versions = {"mis_jpeg_encode_batch": enc, pil_name: lambda: pillow_save(rgbs, use_pool)}
        t = {k: [] for k in versions}
        parts = []
        for _ in range(a.repeats):
            for k, fn in versions.items():
                t[k].append(window(fn, a.iters))
            parts.append(enc.timed())
        v = {"images": len(images), "size": [images[0].shape[1], images[0].shape[0]], "jpeg_bytes": nbytes_out, "equals_pillow": bool(equal),
             "calls": {k: summary(x) for k, x in t.items()},
             "parts": {nm: summary([p[i] for p in parts]) for i, nm in enumerate(PARTS)}}
        mine, pil = v["calls"]["mis_jpeg_encode_batch"], v["calls"][pil_name]
        v["megapixels_per_s"] = sum(im.shape[0] * im.shape[1] for im in images) / mine["median_ms"] / 1e3
        v["over_pillow"] = mine["median_ms"] / pil["median_ms"]
        nbytes = enc.kernel_bytes()
        del enc, versions, images
        torch.cuda.empty_cache()
        if not a.no_kernels:
            v["kernels"] = kernel_stats(a, which, nbytes)
        res["inputs"][which] = v
    if a.parent:
        res["bench_py"] = bench_turns(os.path.abspath(a.parent), a.bench_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
