#!/usr/bin/env python3
"""Writes tests/golden/jpeg_enc: small RGB sources with Pillow's (libjpeg-turbo's) baseline encode of each, the pins of
mis_jpeg_encode.

Needs Pillow, so it runs only where Pillow is installed; the tests read what it wrote.  Deterministic: every source comes from a
seeded generator, and the encoder's options are listed in MANIFEST.json beside the Pillow and libjpeg-turbo versions.

    <name>.npy  the source, uint8 (H, W, 3) RGB
    <name>.jpg  Image.save(quality, subsampling, optimize=False[, restart_marker_blocks])"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_jpeg_fixtures import picture      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_enc")
LIMIT = 64 * 1024
SUBSAMPLING = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}

# (w, h, sampling, quality, restart interval, picture)
FIXTURES = [
    (1, 1, "420", 90, 0, "picture"),
    (8, 8, "444", 90, 0, "picture"),
    (16, 16, "420", 90, 0, "picture"),
    (17, 13, "420", 85, 0, "picture"),
    (9, 17, "420", 85, 0, "picture"),
    (3, 5, "422", 95, 0, "picture"),
    (33, 19, "422", 75, 0, "picture"),
    (50, 40, "420", 95, 0, "picture"),
    (47, 31, "420", 100, 0, "checker"),
    (47, 31, "420", 5, 0, "picture"),
    (300, 20, "420", 90, 0, "columns"),
    (64, 48, "420", 60, 2, "picture"),
    (131, 77, "420", 95, 0, "picture"),
]
MIN_FF = 20     # stuffed bytes the "columns" fixture must hold


def checker(w, h, seed):
    """A 0 / 255 checkerboard (the largest coefficients a block can hold) beside flat 0 and flat 255 areas."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.where((xx + yy) & 1, 255, 0)
    img[:, :w // 4] = 0
    img[:, w // 4:w // 2] = 255
    return np.repeat(img[:, :, None], 3, axis=2).astype(np.uint8)


def columns(w, h, seed):
    """Flat grey with sparse bright columns: long runs of short codes, whose bytes are often FF."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 128, np.uint8)
    for x in rng.choice(w, size=w // 9, replace=False):
        img[:, x] = rng.integers(200, 256, size=3)
    return img


def name_of(w, h, mode, quality, restart, kind):
    return "%dx%d_%s_q%d%s%s" % (w, h, mode, quality, "_dri%d" % restart if restart else "", "" if kind == "picture" else "_" + kind)


def encode(img, mode, quality, restart):
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(quality=quality, subsampling=SUBSAMPLING[mode], optimize=False)
    if restart:
        kw["restart_marker_blocks"] = restart
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue(), kw


def main():
    try:
        import PIL
        from PIL import features
    except ImportError:
        print("Pillow is not installed here: nothing written")
        return 1
    os.makedirs(OUT, exist_ok=True)
    manifest = dict(pillow=PIL.__version__, libjpeg_turbo=features.version("jpg"), fixtures=[])
    makers = dict(picture=picture, checker=checker, columns=columns)
    for seed, (w, h, mode, quality, restart, kind) in enumerate(FIXTURES):
        name = name_of(w, h, mode, quality, restart, kind)
        img = np.ascontiguousarray(makers[kind](w, h, 3000 + seed))
        data, kw = encode(img, mode, quality, restart)
        stuffed = data.count(b"\xff\x00")
        if kind == "columns":
            assert stuffed >= MIN_FF, (name, stuffed)
        assert len(data) <= LIMIT, (name, len(data))
        with open(os.path.join(OUT, name + ".jpg"), "wb") as fh:
            fh.write(data)
        np.save(os.path.join(OUT, name + ".npy"), img)
        assert os.path.getsize(os.path.join(OUT, name + ".npy")) <= LIMIT
        manifest["fixtures"].append(dict(name=name, width=w, height=h, sampling=mode, quality=quality, restart_interval=restart,
                                         picture=kind, options=kw, bytes=len(data), stuffed_ff=stuffed))
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")
    print("wrote %d fixtures to %s" % (len(manifest["fixtures"]), OUT))
    return 0


if __name__ == "__main__":
    sys.exit(main())
