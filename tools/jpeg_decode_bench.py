"""mis_jpeg_decode_batch on the MI355X: config 3's sixteen 4K synthetic frames, encoded here with Pillow (4:2:0, quality 90) once
without restart markers and once with one restart interval per MCU row, decoded in one batch call.

  python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode_v1.json]

What is measured: the call (host clock; it returns synchronised) in alternation with Pillow -- libjpeg-turbo -- decoding the same
sixteen byte strings on sixteen host threads, 7 windows per setting after a warm-up, median and max - min; the call's parts from
mis_jpeg_decode_batch_timed (header pass and entropy decode on the host clock, upload and the two launches between stream events);
the two kernels' times from ONE `rocprofv3 --kernel-trace --stats` run of this script's child mode, with each kernel's bytes
(computed from the frames' geometry) over that time against 8 TB/s.  The decoded pixels are compared with Pillow's before anything
is timed.  Needs a GPU and Pillow: without Pillow nothing can be encoded, the tool says so and measures nothing."""
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

KERNELS = ("jpeg_idct_kernel", "jpeg_color_kernel")
PEAK_TBS = 8.0
VARIANTS = {"no_restart": {}, "restart_per_mcu_row": {"restart_marker_rows": 1}}
THREADS = 16


def encode_frames(workload, opts):
    from PIL import Image
    out = []
    for c in synth.workload(workload):
        bgr = synth.render_frame_gpu(c).cpu().numpy()
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=90, subsampling="4:2:0", **opts)
        out.append(buf.getvalue())
    return out


def pillow_decode(datas, pool):
    from PIL import Image

    def one(d):
        im = Image.open(io.BytesIO(d))
        im.load()
        return im
    return list(pool.map(one, datas))


class Decoder:
    """the batch call on outputs allocated once"""

    def __init__(self, ctx, datas):
        self.ctx, self.datas, self.n = ctx, datas, len(datas)
        self.infos = [isa.jpeg_info(d) for d in datas]
        self.out = [st._empty_image(ctx, i["height"], i["width"], 3, torch.uint8) for i in self.infos]
        self.ptrs = st._c_array(C.c_void_p, (C.cast(C.c_char_p(d), C.c_void_p) for d in datas))
        self.sizes = st._c_array(C.c_size_t, (len(d) for d in datas))
        self.imgs = st._images(self.out)

    def __call__(self):
        self.ctx.check(self.ctx.lib.mis_jpeg_decode_batch(self.ctx.h, self.ptrs, self.sizes, self.n, self.imgs))

    def timed(self):
        ms = (C.c_float * 5)()
        self.ctx.check(self.ctx.lib.mis_jpeg_decode_batch_timed(self.ctx.h, self.ptrs, self.sizes, self.n, self.imgs, ms))
        return list(ms)

    def kernel_bytes(self):
        """bytes each kernel has to move: coefficients in + samples out over the padded planes; samples in + BGR out"""
        idct = color = 0
        for i in self.infos:
            hmax, vmax = max(i["h"]), max(i["v"])
            mx, my = -(-i["width"] // (8 * hmax)), -(-i["height"] // (8 * vmax))
            samples = sum(mx * h * my * v * 64 for h, v in zip(i["h"], i["v"]))
            idct += samples * 3
            color += samples + i["width"] * i["height"] * 3
        return {"jpeg_idct_kernel": idct, "jpeg_color_kernel": color}


def window(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) / iters * 1e3


def summary(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), windows=len(v))


def child(workload, variant, calls):
    ctx = isa.Context(0)
    dec = Decoder(ctx, encode_frames(workload, VARIANTS[variant]))
    for _ in range(calls):
        dec()
    torch.cuda.synchronize()


def kernel_stats(a, variant, nbytes):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--variant", variant, "--kernel-calls", str(a.kernel_calls)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_v1.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--variant", default="no_restart", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    try:
        import PIL
        from PIL import features
    except ImportError:
        print("Pillow is not installed here: the frames cannot be encoded, nothing is measured")
        return 1
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if a.child:
        return child(a.workload, a.variant, a.kernel_calls)
    ctx = isa.Context(0)
    res = {"what": "mis_jpeg_decode_batch of %s's frames (Pillow-encoded 4:2:0 q90) on one MI355X against Pillow %s / libjpeg-turbo %s decoding the same "
                   "byte strings on %d host threads" % (a.workload, PIL.__version__, features.version("jpg"), THREADS),
           "method": "host clock around %d calls, %d windows per setting, the two decoders alternated in one process after a warm-up; parts from "
                     "mis_jpeg_decode_batch_timed (median of the windows' calls); kernels from one rocprofv3 --kernel-trace --stats run per variant" % (a.iters, a.repeats),
           "workload": a.workload, "host_threads": min(THREADS, os.cpu_count() or 1), "variants": {}}
    pool = concurrent.futures.ThreadPoolExecutor(THREADS)
    for variant, opts in VARIANTS.items():
        datas = encode_frames(a.workload, opts)
        dec = Decoder(ctx, datas)
        dec()
        ref = pillow_decode(datas, pool)
        equal = all(np.array_equal(o.cpu().numpy(), np.asarray(r)[:, :, ::-1]) for o, r in zip(dec.out, ref))
        del ref
        versions = {"mis_jpeg_decode_batch": dec, "pillow_%d_threads" % THREADS: lambda: pillow_decode(datas, pool)}
        for fn in versions.values():
            fn()
        t = {k: [] for k in versions}
        parts = []
        for _ in range(a.repeats):
            for k, fn in versions.items():
                t[k].append(window(fn, a.iters))
            parts.append(dec.timed())
        names = ("host_headers_ms", "host_entropy_ms", "upload_ms", "idct_kernel_ms", "color_kernel_ms")
        v = {"frames": len(datas), "size": [dec.infos[0]["width"], dec.infos[0]["height"]], "jpeg_bytes": sum(len(d) for d in datas),
             "restart_interval": dec.infos[0]["restart_interval"], "equals_pillow": bool(equal),
             "calls": {k: summary(x) for k, x in t.items()},
             "parts": {nm: summary([p[i] for p in parts]) for i, nm in enumerate(names)}}
        ours, pil = v["calls"]["mis_jpeg_decode_batch"], v["calls"]["pillow_%d_threads" % THREADS]
        v["frames_per_s"] = len(datas) / ours["median_ms"] * 1e3
        v["over_pillow"] = ours["median_ms"] / pil["median_ms"]
        nbytes = dec.kernel_bytes()
        del dec, versions
        torch.cuda.empty_cache()
        if not a.no_kernels:
            v["kernels"] = kernel_stats(a, variant, nbytes)
        res["variants"][variant] = v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "method")}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
