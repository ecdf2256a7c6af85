"""The affine-partial path's results, bit for bit: tests/golden/affine_bits.json.

  python tools/affine_golden.py [--commit REV] [--out tests/golden/affine_bits.json]

Run once on the MI355X against the library whose bits are to be kept (--commit names it in the file).  Recorded:
  * isa.estimate_affine_partial on every case of every family of tests/refimpl_affine.py (decided by the reference or not), as the
    case stands and again with refine_iters 0 (no LM) and 1 (the stop after one iteration): ok, M as six u64 words, the mask's sha256;
  * one AffineBestOf2NearestMatcher call on refimpl_affine.matcher_batch(): every field of every entry.  The single-problem entry
    runs a problem's whole tail in its replay launch; only the matcher call takes the mask-only and refine-only launches.
Every record carries a sha256 of its inputs, so a drifted generator shows as that and not as a changed result.
tests/test_affine_golden_gpu.py runs record() again and compares.  Needs a GPU."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "affine_bits.json")
REFINE_VARIANTS = ("case", 0, 1)        # the case's own refine_iters, then the LM skipped and stopped after one iteration


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def _words(a):
    return ["%016x" % w for w in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)]


def estimate_records(ctx):
    import image_stitching_amd as isa
    import refimpl_affine as ra
    out = []
    for family in sorted(ra.FAMILIES):
        for case in ra.FAMILIES[family]():
            for variant in REFINE_VARIANTS:
                kw = dict(case["kw"]) if variant == "case" else dict(case["kw"], refine_iters=variant)
                ok, M, mask = isa.estimate_affine_partial(ctx, case["src"], case["dst"], **kw)
                out.append(dict(family=family, name=case["name"], refine_iters=variant,
                                input=_sha(case["src"], case["dst"], repr(sorted(kw.items())).encode()),
                                ok=bool(ok), M=_words(M), mask=_sha(mask)))
    return out


def matcher_record(ctx):
    import image_stitching_amd as isa
    import refimpl_affine as ra
    from image_stitching_amd.stitching import KP_DTYPE
    frames = ra.matcher_batch()["frames"]
    feats = []
    for i, f in enumerate(frames):
        k = np.zeros(len(f["xy"]), KP_DTYPE)
        k["x"], k["y"] = f["xy"][:, 0], f["xy"][:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, f["size"], k, f["desc"], i))
    entries = [dict(src=int(m.src_img_idx), dst=int(m.dst_img_idx), num_inliers=int(m.num_inliers), confidence=_words([m.confidence])[0],
                    H=None if m.H is None else _words(m.H), matches=_sha(np.asarray(m.matches)), inliers_mask=_sha(np.asarray(m.inliers_mask)))
               for m in isa.AffineBestOf2NearestMatcher(ctx)(feats)]
    parts = [x for f in frames for x in (np.asarray(f["size"], np.int64), f["xy"], f["desc"])]
    return dict(input=_sha(*parts), entries=entries)


def record(ctx):
    return dict(estimate=estimate_records(ctx), matcher=matcher_record(ctx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="the commit of the library the bits are recorded at")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import image_stitching_amd as isa
    ctx = isa.Context(0)
    rec = dict(recorded_at=a.commit, **record(ctx))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write('{"recorded_at": %s,\n "estimate": [\n  ' % json.dumps(rec["recorded_at"]))
        fh.write(",\n  ".join(json.dumps(r) for r in rec["estimate"]))
        fh.write('\n ],\n "matcher": {"input": %s, "entries": [\n  ' % json.dumps(rec["matcher"]["input"]))
        fh.write(",\n  ".join(json.dumps(e) for e in rec["matcher"]["entries"]))
        fh.write("\n ]}\n}\n")
    print("%d estimate records, %d matcher entries -> %s" % (len(rec["estimate"]), len(rec["matcher"]["entries"]), a.out))


if __name__ == "__main__":
    main()
