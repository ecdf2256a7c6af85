"""GPU parity of ORB on inputs that fill fast_nms_kernel's queue: the survivor list and the tile histogram share the LDS of the gray
tile, which is safe only if nothing reads the tile behind the arc evaluation.  On uniform byte noise nearly every pixel passes stage A,
so the queue, the score map and the aliased arrays are all in use at once; every stage equals the CPU oracle bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST_T = 20


def noise_frame(w, h, seed, blocks=True):
    """Uniform u8 noise (B = G = R, so the gray level 0 is the noise itself) with a few flat blocks pasted in."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if blocks:
        for (x, y, v) in ((40, 30, 200), (130, 100, 17), (w - 20, h - 18, 90), (0, 70, 255)):
            g[y:y + 16, x:x + 16] = v
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def stage_a_pass_rate(gray, t):
    """Share of the scored pixels (3 or more from the edge) for which both the vertical and the horizontal pair of circle pixels hold
    one that differs from the centre by more than t: the condition under which fast_nms_kernel queues a pixel."""
    g = gray.astype(np.int32)
    c = g[3:-3, 3:-3]
    dv = np.maximum(np.abs(g[6:, 3:-3] - c), np.abs(g[:-6, 3:-3] - c))
    dh = np.maximum(np.abs(g[3:-3, 6:] - c), np.abs(g[3:-3, :-6] - c))
    return float(np.mean(np.minimum(dv, dh) > t))


def check_frame(finder, orb, frame):
    import torch
    feats = finder.detect(torch.from_numpy(frame).cuda())
    okps, odesc = orb.run(frame)
    for l in range(orb.params.nlevels):
        assert np.array_equal(finder.debug_level(l, 0), orb.level_gray(l)), "gray level %d" % l
        assert np.array_equal(finder.debug_level(l, 1), orb.level_nms(l)), "nms level %d" % l
        assert np.array_equal(finder.debug_level(l, 2), orb.level_blur(l)), "blur level %d" % l
    kps, desc = feats.download()
    assert len(kps) == len(okps)
    for f in ("octave", "x", "y", "size", "response", "angle"):
        assert np.array_equal(kps[f], okps[f]), f
    assert np.array_equal(desc, odesc)
    return kps, desc


def test_noise_fills_the_queue_default_params(ctx, oracle_mod):
    """256 x 192 noise, default parameters: P(|a - b| <= 20) = 0.154 for uniform bytes, so a pixel passes stage A with probability
    (1 - 0.154^2)^2 = 0.95 -- checked on the input itself, without the GPU code -- and every 64 x 64 tile queues nearly all of its
    66 x 66 scored pixels."""
    import image_stitching_amd as isa
    w, h = 256, 192
    frame = noise_frame(w, h, 1)
    assert stage_a_pass_rate(frame[:, :, 0], FAST_T) >= 0.9
    finder = isa.OrbFeatureFinder(ctx, (w, h))
    kps, _ = check_frame(finder, oracle_mod.Orb(w, h), frame)
    assert len(kps) > 1000


def test_finder_reused_after_a_dense_frame(ctx, oracle_mod):
    """The same finder on a dense frame, then on a sparse and on a flat one: what the dense frame left in the workspace is inert."""
    import image_stitching_amd as isa
    w, h = 256, 192
    finder = isa.OrbFeatureFinder(ctx, (w, h))
    orb = oracle_mod.Orb(w, h)
    check_frame(finder, orb, noise_frame(w, h, 2))
    sparse = np.full((h, w, 3), 90, np.uint8)
    sparse[40:80, 50:120] = (200, 30, 60)
    sparse[100:120, 20:40] = (10, 220, 130)
    kps, desc = check_frame(finder, orb, sparse)
    import torch
    fresh = isa.OrbFeatureFinder(ctx, (w, h)).detect(torch.from_numpy(sparse).cuda()).download()
    assert np.array_equal(fresh[0], kps) and np.array_equal(fresh[1], desc) and 0 < len(kps) < 200
    kps, _ = check_frame(finder, orb, np.full((h, w, 3), 128, np.uint8))
    assert len(kps) == 0


# (w, h) with partial tiles in both directions; the pattern's reach is 28 for patch 40, 22 for 32, 21 for 30, 10 for 14
@pytest.mark.parametrize("kw", [dict(edge_threshold=31, patch_size=30), dict(patch_size=32), dict(edge_threshold=0, patch_size=14, score_type=1),
                                dict(fast_threshold=5, nfeatures=1500, nlevels=3)],
                         ids=["edge31-patch30", "patch32", "edge0-patch14-fastscore", "fast5-3levels"])
def test_noise_other_params(ctx, oracle_mod, kw):
    """Dense frames at other parameter sets: a wide and a zero edge threshold, patterns of other reaches, the FAST score as the
    response, a low FAST threshold (every scored pixel queued: the queue at its capacity)."""
    import image_stitching_amd as isa
    w, h = 200, 150
    frame = noise_frame(w, h, 3, blocks=False)
    if kw.get("fast_threshold") == 5:
        assert stage_a_pass_rate(frame[:, :, 0], 5) >= 0.99
    finder = isa.OrbFeatureFinder(ctx, (w, h), isa.stitching.orb_params(**kw))
    check_frame(finder, oracle_mod.Orb(w, h, oracle_mod.orb_default_params(**kw)), frame)
