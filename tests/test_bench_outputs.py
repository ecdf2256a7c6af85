"""bench.py --dump-outputs: what the timed path returned in its last step, as float32 / float64 .npy files of at most 64 MB in
all (large outputs as a fixed, seeded sample of their rows), the same files for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


class _Feats:
    def __init__(self, kps, desc):
        self.kps, self.desc = kps, desc

    def download(self):
        return self.kps, self.desc


class _Pairs:
    """The PairwiseMatches interface job_outputs reads: n, and entry i * n + j as a MatchesInfo."""

    def __init__(self, n, entries):
        self.n, self.entries = n, entries

    def __getitem__(self, k):
        from image_stitching_amd.stitching import MatchesInfo
        return self.entries.get(k, MatchesInfo())


def _fake_out(h, w, n=3, kps_per_frame=500):
    from image_stitching_amd.stitching import DMATCH_DTYPE, KP_DTYPE, MatchesInfo
    rng = np.random.default_rng(7)
    feats = []
    for _ in range(n):
        k = np.zeros(kps_per_frame, KP_DTYPE)
        for c in ("x", "y", "size", "angle", "response"):
            k[c] = rng.random(kps_per_frame, np.float32) * 100
        k["octave"] = rng.integers(0, 8, kps_per_frame)
        feats.append(_Feats(k, rng.integers(0, 256, (kps_per_frame, 32)).astype(np.uint8)))
    entries = {}
    for i in range(n):
        for j in range(n):
            if i != j:
                m = np.zeros(40 + i + j, DMATCH_DTYPE)
                m["query_idx"], m["train_idx"], m["distance"] = np.arange(len(m)), np.arange(len(m))[::-1], rng.random(len(m), np.float32)
                H = np.eye(3) * (i + 1) if i < j else None
                entries[i * n + j] = MatchesInfo(i, j, m, (np.arange(len(m)) % 2).astype(np.uint8), len(m) // 2, H, 0.5)
    conf = torch.from_numpy(rng.random((n, n)))
    return {"pano": torch.from_numpy(rng.integers(-255, 256, (h, w, 3)).astype(np.int16)),
            "mask": torch.from_numpy(rng.integers(0, 2, (h, w)).astype(np.uint8) * 255),
            "indices": list(range(n)), "confidence": conf, "matches": _Pairs(n, entries), "features": feats,
            "pano_size": (w, h), "num_bands": 5}


def test_small_outputs_are_written_whole(tmp_path):
    import bench
    out = _fake_out(60, 90)
    arrays = bench.job_outputs(out)
    bench.dump_outputs(str(tmp_path), arrays)
    got = _load(str(tmp_path))
    for a in got.values():
        assert a.dtype in (np.float32, np.float64)
    assert np.array_equal(got["pano"], out["pano"].numpy().reshape(-1, 3)) and np.array_equal(got["mask"], out["mask"].numpy().reshape(-1))
    assert np.array_equal(got["pano_sample"], np.arange(60 * 90))
    assert got["pano_size"].tolist() == [90, 60] and got["num_bands"].tolist() == [5] and got["indices"].tolist() == [0, 1, 2]
    assert np.array_equal(got["confidence"], out["confidence"].numpy())
    k0, d0 = out["features"][1].download()
    rows = got["keypoints"][:, 0] == 1
    assert got["feature_counts"].tolist() == [500] * 3 and rows.sum() == 500
    assert np.array_equal(got["keypoints"][rows, 1], k0["x"]) and np.array_equal(got["keypoints"][rows, 6], k0["octave"])
    assert np.array_equal(got["descriptors"][rows], d0)
    m = out["matches"][0 * 3 + 2]
    sel = (got["matches"][:, 0] == 0) & (got["matches"][:, 1] == 2)
    assert np.array_equal(got["matches"][sel][:, 2], m.matches["query_idx"]) and np.array_equal(got["matches"][sel][:, 5], m.inliers_mask)
    assert got["match_counts"][0, 2] == len(m.matches) and got["num_inliers"][0, 2] == m.num_inliers
    assert np.array_equal(got["homographies"][0, 2], m.H) and got["has_homography"][0, 2] == 1
    assert not got["homographies"][2, 0].any() and got["has_homography"][2, 0] == 0
    assert all(np.isfinite(a).all() for a in got.values())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    import bench
    out = _fake_out(700, 1000)
    arrays = bench.job_outputs(out)
    budget = {"pano": 2 * 10 ** 6, "keypoint": 40000, "match": 2000}
    n1 = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=3 * 10 ** 6, group_budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), bench.job_outputs(out), budget=3 * 10 ** 6, group_budget=budget)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert n1 <= 3 * 10 ** 6 and sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 3 * 10 ** 6
    idx = a["pano_sample"].astype(np.int64)
    assert 0 < len(idx) < 700 * 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["pano"], out["pano"].numpy().reshape(-1, 3)[idx]) and np.array_equal(a["mask"], out["mask"].numpy().reshape(-1)[idx])
    kidx = a["keypoint_sample"].astype(np.int64)
    assert len(kidx) < 1500 and np.array_equal(a["keypoints"], arrays["keypoints"][kidx]) and np.array_equal(a["descriptors"], arrays["descriptors"][kidx])
    assert len(a["match_sample"]) < len(arrays["matches"])
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), arrays, budget=10 ** 6, group_budget=budget)
    bad = dict(arrays, confidence=np.full((3, 3), np.nan))
    with pytest.raises(ValueError, match="confidence"):
        bench.dump_outputs(str(tmp_path / "d"), bad, budget=3 * 10 ** 6, group_budget=budget)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_what_the_job_computes(tmp_path, ctx):
    """Two bench.py runs with different step counts write the same files, and they are the outputs of the job run here."""
    import bench
    import image_stitching_amd as isa
    import synth
    from image_stitching_amd.distributed import StitchJob
    dirs = []
    for steps in (1, 3):
        d = str(tmp_path / ("s%d" % steps))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--workload", "config2",
                            "--no-cpu-baseline", "--no-cpp-host", "--roofline-launches", "4", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
        assert res["steps"] == steps and res["ms_per_step"] > 0
        dirs.append(_load(d))
    a, b = dirs
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
    cams = synth.workload("config2")
    job = StitchJob(ctx, (cams[0]["width"], cams[0]["height"]), cams, config=isa.StitchConfig.hot_path(features_type="orb"))
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    here = bench.job_outputs(job.run(frames))
    for g, names in bench.DUMP_GROUPS.items():
        idx = a[g + "_sample"].astype(np.int64)
        for nm in names:
            assert np.array_equal(a[nm], here.pop(nm)[idx]), nm
    for nm, v in here.items():
        assert np.array_equal(a[nm], v), nm
