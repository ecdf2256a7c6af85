"""range_width and pair masks, the parts that need no device: selected_pairs against the definition (both frames with keypoints,
the strict upper triangle of the mask, j < i + range_width), the config check, and the engine capability check of StitchJob."""
import numpy as np
import pytest


def _brute(counts, width, mask):
    n = len(counts)
    out = []
    for i in range(n):
        for j in range(n):
            if not i < j:
                continue
            if counts[i] <= 0 or counts[j] <= 0:
                continue
            if mask is not None and mask[i][j] == 0:
                continue
            if width != -1 and not j < i + width:
                continue
            out.append((i, j))
    return out


def test_selected_pairs_vs_definition():
    from image_stitching_amd import selected_pairs
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 6, 9):
        for trial in range(6):
            counts = [int(c) for c in rng.integers(0, 4, n) * rng.integers(0, 500, n)]      # about a quarter of the frames empty
            if trial == 0:
                counts = [100] * n
            for width in (-1, 1, 2, 5, n + 3):
                for mask in (None, rng.integers(0, 2, (n, n)).astype(np.uint8), (rng.integers(0, 3, (n, n)) * 100).astype(np.int32)):
                    got = selected_pairs(counts, width, mask)
                    assert got == _brute(counts, width, mask), (counts, width, mask)
                    assert got == sorted(got)                        # row-major: the order the shards are dealt in
                    if mask is not None:
                        # only the strict upper triangle is read: the diagonal and the lower triangle change nothing
                        other = mask.copy()
                        other[np.tril_indices(n)] = 1 - (other[np.tril_indices(n)] != 0)
                        assert selected_pairs(counts, width, other) == got
    full = [50] * 6
    assert len(selected_pairs(full)) == 15
    assert len(selected_pairs(full, 3)) == 9
    assert selected_pairs(full, 2) == [(i, i + 1) for i in range(5)]
    assert selected_pairs(full, 1) == []
    assert selected_pairs(full, 9) == selected_pairs(full, -1)
    m = np.zeros((6, 6), np.uint8)
    m[5, 0] = m[2, 2] = 1
    assert selected_pairs(full, -1, m) == []
    m[0, 5] = 1
    assert selected_pairs(full, -1, m) == [(0, 5)]
    assert selected_pairs(full, 4, m) == []


@pytest.mark.parametrize("bad", [0, -2, -100, 2.5, "3", None, True])
def test_config_refuses_bad_range_width_before_device_work(bad):
    """ctx None: anything that touched the device would fail otherwise than by ValueError"""
    from image_stitching_amd.distributed import HipEngine, StitchJob
    from image_stitching_amd.stitching import StitchConfig, Stitcher, check_range_config
    cfg = StitchConfig(range_width=bad)
    for make in (lambda: check_range_config(cfg), lambda: Stitcher(None, (640, 360), cfg), lambda: HipEngine(None, (640, 360), cfg),
                 lambda: StitchJob(None, (640, 360), [], config=cfg)):
        with pytest.raises(ValueError, match="range_width"):
            make()


def test_config_accepts_widths_and_presets_are_unchanged():
    from image_stitching_amd.stitching import StitchConfig, check_range_config
    assert StitchConfig().range_width == -1 and StitchConfig.hot_path().range_width == -1 and StitchConfig.reference().range_width == -1
    for w in (-1, 1, 2, 5, 1000):
        assert check_range_config(StitchConfig.hot_path(range_width=w)) == w
    assert check_range_config(StitchConfig(range_width=np.int64(3))) == 3


class _PlainEngine:
    """an engine of before range_width: it says nothing about the selection, so it matches all pairs"""
    warp_type = "spherical"


def test_job_refuses_engine_without_range_width():
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    cams = [synth.make_camera(640, 360, 60.0, 13.0 * i) for i in range(4)]
    job = StitchJob(None, (640, 360), cams, engine=_PlainEngine(), config=StitchConfig.hot_path())      # -1 is what it does
    assert job.cfg.range_width == -1
    for w in (1, 3):
        with pytest.raises(NotImplementedError, match="range_width"):
            StitchJob(None, (640, 360), cams, engine=_PlainEngine(), config=StitchConfig.hot_path(range_width=w))
    declared = _PlainEngine()
    declared.range_width = 3
    assert StitchJob(None, (640, 360), cams, engine=declared, config=StitchConfig.hot_path(range_width=3)).cfg.range_width == 3
    with pytest.raises(NotImplementedError, match="range_width"):
        StitchJob(None, (640, 360), cams, engine=declared, config=StitchConfig.hot_path())


def test_oracle_engine_is_refused_for_a_range_width():
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = [synth.make_camera(640, 360, 60.0, 13.0 * i) for i in range(4)]
    cfg = StitchConfig.hot_path(range_width=2)
    with pytest.raises(NotImplementedError, match="range_width"):
        StitchJob(None, (640, 360), cams, engine=OracleEngine((640, 360), config=cfg), config=cfg)
    StitchJob(None, (640, 360), cams, engine=OracleEngine((640, 360)), config=StitchConfig.hot_path())
