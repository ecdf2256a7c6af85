#!/usr/bin/env python3
"""Writes tests/golden/jpeg: small baseline JPEG streams with Pillow's (libjpeg-turbo's) decode of each, the pins of mis_jpeg_decode.

Needs Pillow, so it runs only where Pillow is installed; the tests read what it wrote.  Deterministic: every image comes from a
seeded generator, and the encoder's options are listed in MANIFEST.json beside the Pillow and libjpeg-turbo versions.

    decode set   <name>.jpg + <name>.npy (RGB, or one plane for the grey file)
    refusal set  <name>.jpg + the code and the cause the library must name
    job set      job/<k>.jpg, job/<k>.npz (the decode, compressed) and job/<k>.txt (the camera): three 480 x 270 frames of the
                 sweep tests/test_host_cpp.py::_write_job renders"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")
LIMIT = 64 * 1024

# (w, h, mode / sampling, options)
DECODE = [
    (8, 8, "444", dict(quality=90)),
    (16, 16, "444", dict(quality=90)),
    (1, 1, "420", dict(quality=90)),
    (17, 13, "420", dict(quality=85)),
    (33, 19, "422", dict(quality=75)),
    (5, 3, "420", dict(quality=95)),
    (3, 5, "422", dict(quality=95)),
    (7, 9, "420", dict(quality=50)),
    (64, 48, "420", dict(quality=60, restart_marker_blocks=2)),
    (131, 77, "420", dict(quality=92, restart_marker_blocks=3)),
    (47, 31, "420", dict(quality=30, restart_marker_rows=1)),
    (40, 24, "grey", dict(quality=80)),
    (47, 31, "420", dict(quality=100)),
    (47, 31, "420", dict(quality=5, restart_marker_blocks=1)),
    (47, 31, "420", dict(qtables=[[255] * 64, [255] * 64])),
    (47, 31, "420", dict(qtables=[[1] * 64, [1] * 64])),
    (47, 31, "420", dict(quality=85, optimize=True)),
]
SUBSAMPLING = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}


def picture(w, h, seed, grey=False):
    """A ramp, a few hard-edged rectangles and noise: smooth areas, saturated edges (ringing past 0 and 255) and texture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 255 // max(w + h - 2, 1))], axis=-1).astype(np.int64)
    for _ in range(4):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = x0 + int(rng.integers(1, max(w // 2, 2))), y0 + int(rng.integers(1, max(h // 2, 2)))
        img[y0:y1, x0:x1] = rng.choice([0, 255], size=3)
    img += rng.integers(-24, 25, size=img.shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[:, :, 1].copy() if grey else img


def name_of(w, h, mode, opts):
    tags = []
    for k, v in opts.items():
        if k == "quality":
            tags.append("q%d" % v)
        elif k == "restart_marker_blocks":
            tags.append("dri%d" % v)
        elif k == "restart_marker_rows":
            tags.append("rows%d" % v)
        elif k == "qtables":
            tags.append("qt%d" % v[0][0])
        elif k == "optimize":
            tags.append("opt")
    return "%dx%d_%s_%s" % (w, h, mode, "_".join(tags))


def encode(img, mode, opts):
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(opts)
    if mode in SUBSAMPLING:
        kw["subsampling"] = SUBSAMPLING[mode]
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def write(path, data):
    assert len(data) <= LIMIT, (path, len(data))
    with open(path, "wb") as fh:
        fh.write(data)


def main():
    try:
        import PIL
        from PIL import Image, features
    except ImportError:
        print("Pillow is not installed here: nothing written")
        return 1
    os.makedirs(os.path.join(OUT, "job"), exist_ok=True)
    manifest = dict(pillow=PIL.__version__, libjpeg_turbo=features.version("jpg"), decode=[], refuse=[], job=[])
    for seed, (w, h, mode, opts) in enumerate(DECODE):
        name = name_of(w, h, mode, opts)
        data = encode(picture(w, h, 1000 + seed, grey=mode == "grey"), mode, opts)
        px = pil_decode(data)
        assert px.shape[:2] == (h, w)
        write(os.path.join(OUT, name + ".jpg"), data)
        np.save(os.path.join(OUT, name + ".npy"), px)
        assert os.path.getsize(os.path.join(OUT, name + ".npy")) <= LIMIT
        manifest["decode"].append(dict(name=name, width=w, height=h, sampling=mode, options=opts))
    # refusals
    base = picture(47, 31, 2000)
    write(os.path.join(OUT, "refuse_progressive.jpg"), encode(base, "420", dict(quality=85, progressive=True)))
    manifest["refuse"].append(dict(name="refuse_progressive", code="MIS_E_UNSUPPORTED", cause="SOF2"))
    buf = io.BytesIO()
    Image.fromarray(base).convert("CMYK").save(buf, "JPEG", quality=85)
    write(os.path.join(OUT, "refuse_cmyk.jpg"), buf.getvalue())
    manifest["refuse"].append(dict(name="refuse_cmyk", code="MIS_E_UNSUPPORTED", cause="4 components"))
    whole = open(os.path.join(OUT, name_of(17, 13, "420", dict(quality=85)) + ".jpg"), "rb").read()
    write(os.path.join(OUT, "refuse_truncated.jpg"), whole[:len(whole) // 2])
    manifest["refuse"].append(dict(name="refuse_truncated", code="MIS_E_INVALID", cause="truncated"))
    # the job: test_host_cpp._write_job's three-frame 480 x 270 sweep
    import oracle
    import synth
    from test_host_cpp import _desc
    w, h = 480, 270
    frames, descs = [], []
    for i in range(3):
        c = synth.make_camera(w, h, 60.0, 14.0 * i - 10.0, 0.5 * (i - 1), -0.3 * i)
        R_sensor = oracle.camera_rehand(c["R"], False)
        c_eff = dict(c)
        c_eff["R"] = oracle.camera_rehand(R_sensor, False)
        frames.append(synth.render_frame(c_eff)[:, :, ::-1])       # BGR -> RGB for the encoder
        descs.append(_desc(c, R_sensor))
    quality = next(q for q in range(100, 0, -1) if all(len(encode(f, "420", dict(quality=q))) <= LIMIT for f in frames))
    for i, (f, d) in enumerate(zip(frames, descs)):
        data = encode(np.ascontiguousarray(f), "420", dict(quality=quality))
        write(os.path.join(OUT, "job", "%d.jpg" % (i + 1)), data)
        np.savez_compressed(os.path.join(OUT, "job", "%d.npz" % (i + 1)), rgb=pil_decode(data))
        with open(os.path.join(OUT, "job", "%d.txt" % (i + 1)), "w") as fh:
            fh.write(d)
        manifest["job"].append(dict(name="job/%d" % (i + 1), width=w, height=h, sampling="420", options=dict(quality=quality),
                                    npz_bytes=os.path.getsize(os.path.join(OUT, "job", "%d.npz" % (i + 1)))))
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")
    print("wrote %d decode, %d refusal and %d job fixtures to %s (job quality %d)" % (len(manifest["decode"]), len(manifest["refuse"]), len(manifest["job"]), OUT, quality))
    return 0


if __name__ == "__main__":
    sys.exit(main())
