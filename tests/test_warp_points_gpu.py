"""mis_warper_warp_points on the device: warp_points_kernel's bits equal the host loop's bits, for all eleven kinds, both
directions, point counts around the wave and workgroup sizes, and the special points (poles, z = 0, the polar kinds' origin, NaN,
+-inf) among ordinary ones.  Compared as bit patterns, NaN positions equal (payloads aside)."""
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_affine_family as ra
import refimpl_warp_backward as rb
import image_stitching_amd as isa

pytestmark = pytest.mark.gpu
W, H = 96, 54
COUNTS = (1, 63, 64, 65, 4099)


def special_points(scale):
    ps = math.pi * scale
    big = np.finfo(np.float32).max
    return np.array([(W / 2, H / 2), (0, 0), (W - 1, H - 1), (W / 2, -1e6), (W / 2, 1e6), (-1e6, H / 2), (1e6, H / 2), (0, ps), (0, 0), (ps, ps / 2),
                     (-ps, ps / 2), (ps / 2, ps / 2), (-ps / 2, 0), (1e-30, -1e-30), (np.nan, 0), (0, np.nan), (np.nan, np.nan), (np.inf, 0), (0, -np.inf),
                     (np.inf, np.inf), (-np.inf, np.inf), (big, big), (-big, big), (0.5, 0.5), (-0.0, 0.0)], np.float32)


def points(n, scale, seed):
    rng = np.random.default_rng(seed)
    sp = special_points(scale)
    p = np.empty((n, 2), np.float32)
    p[:, 0] = rng.uniform(-4 * scale, 4 * scale, n)
    p[:, 1] = rng.uniform(-4 * scale, 4 * scale, n)
    k = min(n, len(sp))
    p[rng.permutation(n)[:k]] = sp[rng.permutation(len(sp))[:k]] if n < len(sp) else sp
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("name", list(rb.KINDS))
def test_device_points_equal_host_points_bit_for_bit(ctx, name):
    kind = rb.KINDS[name]
    if kind == rb.AFFINE:
        cams = [(K, Hm, s) for _, K, Hm, s in ra.warp_cases(W, H)[4:7]]
    else:
        cams = [ri.camera(W, H, *g[1:]) for g in ri.WARP_GEOMS if g[0] in ("front", "seam+", "pitch+85", "roll-30", "hfov150")]
    for ci, (K, R, scale) in enumerate(cams):
        dev, host = isa.RotationWarper(ctx, scale, kind), isa.RotationWarper(None, scale, kind)
        for n in COUNTS:
            for backward in (False, True):
                p = points(n, scale, 100 * ci + n)
                d, h = dev.warp_points(p, K, R, backward), host.warp_points(p, K, R, backward)
                assert d.shape == (n, 2) and same_bits(d, h), (name, ci, n, backward, np.flatnonzero((d != h).any(1))[:5])


def test_no_points_is_a_no_op_and_refusals_carry_a_text(ctx):
    K, R, scale = ri.camera(W, H, 60.0, 0.0)
    w = isa.RotationWarper(ctx, scale, isa.WARP_SPHERICAL)
    assert w.warp_points(np.zeros((0, 2), np.float32), K, R).shape == (0, 2)
    with pytest.raises(isa.stitching.MisError) as e:
        isa.RotationWarper(ctx, -1.0, isa.WARP_SPHERICAL).warp_points([(1, 2)], K, R)
    assert e.value.code == isa._capi.MIS_E_INVALID
    u, v = w.warpPoint((10.5, 20.25), K, R)
    x, y = w.warpPointBackward((u, v), K, R)
    assert abs(x - 10.5) < 1e-2 and abs(y - 20.25) < 1e-2
