"""dev_math.h in a kernel against dev_math.h on the host (test_dev_math_cpu.py pins the host): every function the test aids
reach gives the host's result in every bit on the device, NaNs compared as NaNs.  Inputs per function: every float32 within 4096
ulps of each branch point of its code, 2^22 random bit patterns inside its domain, and the SPECIALS of test_mercator_gpu.py.  The
raw sqrtf(x), 1.0f / x and a / b are compared with numpy float32 as well: the direct test of the header's sentence that the
device's division and square root are correctly rounded, and of subnormals not being flushed.

A function's domain is where its C is defined: the float -> integer conversions of mis_sincosf (|x| < 2^31 here; the stated range is
8192), mis_round_f, mis_floor_f and mis_round_d (|v| < 2^31) are undefined beyond, on the host as in the standard, so inputs
outside are not compared; mis_round_sat_f, which exists for those inputs, takes everything."""
import math

import numpy as np
import pytest

import devmath as dm
from test_mercator_gpu import SPECIALS

pytestmark = pytest.mark.gpu

F = np.float32
N_RANDOM = 1 << 22
PI4 = math.pi / 4
TINY = 1.1754944e-38             # 2^-126, the subnormal threshold
SPEC = np.array(SPECIALS, F)
INT_RANGE = lambda v: np.abs(v) < 2147483648.0       # noqa: E731  (NaN: False)
ANY = None

STATED = {"sin": lambda v: np.abs(v) <= 8192.0, "cos": lambda v: np.abs(v) <= 8192.0}       # where the random patterns are drawn, if narrower

# name -> (branch points, domain of every input)
UNARY = {
    "sin": ([k * PI4 for k in range(-4, 9)] + [8192.0, -8192.0], INT_RANGE),
    "cos": ([k * PI4 for k in range(-4, 9)] + [8192.0, -8192.0], INT_RANGE),
    "acos": ([s * c for s in (1, -1) for c in (1e-4, 0.5, 1.0)], ANY),
    "asin": ([s * c for s in (1, -1) for c in (1e-4, 0.5, 1.0)], ANY),
    "atan": ([s * c for s in (1, -1) for c in (0.4142135, 2.4142135)], ANY),
    "log": ([TINY, 0.0, 0.70710678, 1.0, 1.4142135], ANY),
    "exp": ([-87.33654, -103.27893, 88.72284, 0.0], ANY),
    "sqrt": ([TINY, 0.0, 4 * TINY], ANY),
    "rcp": ([TINY, -TINY, 0.0, 8.507059e37, -8.507059e37, 1.7014118e38], ANY),       # 1 / x is subnormal beyond 2^126, x itself below 2^-126
    "round_f": ([2147483648.0, -2147483648.0, 0.5, -0.5, 8388608.0], INT_RANGE),
    "round_sat_f": ([2147483648.0, -2147483648.0, 0.5, -0.5, 8388608.0], ANY),
    "floor_f": ([2147483648.0, -2147483648.0, 0.0, 1.0, -1.0, 8388608.0, -8388608.0], INT_RANGE),
}


def _host_and_device(ctx, name, a, b=None):
    host, dev = dm.call(name, a, b), dm.call(name, a, b, ctx=ctx)
    bad = ~dm.same_bits(host, dev)
    assert not bad.any(), (name, int(bad.sum()), np.asarray(a)[bad][:6], None if b is None else np.asarray(b)[bad][:6], host[bad][:6], dev[bad][:6])
    return dev


def _inside(x, keep):
    if keep is None:
        return x
    with np.errstate(invalid="ignore"):
        return x[keep(x)]


@pytest.mark.parametrize("name", sorted(UNARY))
def test_unary_device_bits_equal_host_bits(ctx, name):
    points, keep = UNARY[name]
    rng = np.random.default_rng(sorted(UNARY).index(name) + 100)
    x = np.concatenate([_inside(dm.around(points), keep), dm.random_bits(rng, N_RANDOM, STATED.get(name, keep)), _inside(SPEC, keep), _inside(-SPEC, keep)])
    if name in ("acos", "asin"):            # half of the random patterns inside [-1, 1], where the polynomials are
        x = np.concatenate([x, dm.random_bits(rng, N_RANDOM // 2, lambda v: np.abs(v) <= 1.0)])
    if name in ("round_f", "round_sat_f"):  # the ties
        x = np.concatenate([x, (np.arange(-70000, 70000) + 0.5).astype(F)])
    dev = _host_and_device(ctx, name, x)
    if name in ("sqrt", "rcp"):
        with np.errstate(all="ignore"):
            want = np.sqrt(x) if name == "sqrt" else F(1.0) / x
            bad = ~dm.same_bits(dev, want)
            assert not bad.any(), (name, int(bad.sum()), x[bad][:6], dev[bad][:6], want[bad][:6])
            sub = (x != 0) & (np.abs(x) < F(TINY))
            assert sub.sum() > 10000 and (dev[sub & (x > 0)] != (0 if name == "sqrt" else np.inf)).any()        # subnormal inputs are not read as zero


def _pairs_about(points, others):
    """(y, x): y within 4096 ulps of c * x for every branch point c of the quotient and every x of `others`"""
    ys, xs = [], []
    for c in points:
        for x0 in others:
            y = dm.around([c * x0])
            ys.append(y)
            xs.append(np.full(y.size, x0, F))
    return np.concatenate(ys), np.concatenate(xs)


def _special_grid():
    s = np.concatenate([SPEC, -SPEC])
    return np.repeat(s, s.size), np.tile(s, s.size)


@pytest.mark.parametrize("name", ["atan2", "fast_atan2", "div"])
def test_binary_device_bits_equal_host_bits(ctx, name):
    """atan2: the quotient about the inner atan's switches 0.4142135 and 2.4142135 (and their negatives); fast_atan2: |y| about
    |x|, the ax >= ay switch; the division: quotients about the subnormal threshold and the overflow, subnormal operands."""
    rng = np.random.default_rng({"atan2": 21, "fast_atan2": 22, "div": 23}[name])
    xs = [1.0, -1.0, 3.0, -0.37, 1e-20, 1e20]
    if name == "atan2":
        y, x = _pairs_about([0.4142135, 2.4142135, -0.4142135, -2.4142135, 0.0], xs)
    elif name == "fast_atan2":
        y, x = _pairs_about([1.0, -1.0, 0.0], xs)
        fy, fx = dm.fast_atan2_inputs(rng, 1 << 18)
        y, x = np.concatenate([y, fy]), np.concatenate([x, fx])
    else:
        y, x = dm.ieee_pairs(rng, 1 << 18)
        ty, tx = _pairs_about([TINY, -TINY], [1.0, -3.0, 1.0000001])
        oy, ox = _pairs_about([3.4028235e38], [1.0])
        y, x = np.concatenate([y, ty, oy]), np.concatenate([x, tx, ox])
    gy, gx = _special_grid()
    y = np.concatenate([y, dm.random_bits(rng, N_RANDOM), gy])
    x = np.concatenate([x, dm.random_bits(rng, N_RANDOM), gx])
    dev = _host_and_device(ctx, name, y, x)
    if name == "div":
        with np.errstate(all="ignore"):
            want = y / x
            bad = ~dm.same_bits(dev, want)
            assert not bad.any(), (int(bad.sum()), y[bad][:6], x[bad][:6], dev[bad][:6], want[bad][:6])
            assert ((want != 0) & (np.abs(want) < F(TINY))).sum() > 30000          # subnormal quotients were asked for, and kept
    if name == "fast_atan2":
        bad = ~dm.same_bits(dev, dm.fast_atan2_f32(y, x))
        assert not bad.any(), (int(bad.sum()), y[bad][:6], x[bad][:6])


def test_integer_functions_device_equal_host(ctx):
    """mis_sat_short about both bounds and on random integers; the three border maps on the cases of the host test and on random
    (p, len) with len up to 2^20 (mis_reflect1 on its domain [-len, 2 len))."""
    rng = np.random.default_rng(31)
    v = np.concatenate([np.arange(-32768 - 4096, -32768 + 4096), np.arange(32767 - 4096, 32767 + 4096), rng.integers(-2 ** 31, 2 ** 31, 1 << 20),
                        [-2 ** 31, 2 ** 31 - 1, 0]]).astype(np.int32)
    dev = _host_and_device(ctx, "sat_short", v)
    assert np.array_equal(dev, np.clip(v, -32768, 32767))
    c = dm.reflect_cases()
    n = np.concatenate([c[:, 1], rng.integers(1, 1 << 20, 1 << 20)]).astype(np.int32)
    p = np.concatenate([c[:, 0], rng.integers(-(1 << 30), 1 << 30, 1 << 20)]).astype(np.int32)
    d101, dsym = _host_and_device(ctx, "reflect101", p, n), _host_and_device(ctx, "reflect", p, n)
    assert np.array_equal(d101[: len(c)], c[:, 2]) and np.array_equal(dsym[: len(c)], c[:, 3])
    assert d101.min() >= 0 and dsym.min() >= 0 and (d101 < n).all() and (dsym < n).all()
    p1 = (rng.integers(0, 3 << 20, n.size) % (3 * n.astype(np.int64)) - n).astype(np.int32)         # [-len, 2 len)
    d1 = _host_and_device(ctx, "reflect1", p1, n)
    assert np.array_equal(d1, dm.call("reflect", p1, n))


def test_double_functions_device_bits_equal_host_bits(ctx):
    """mis_log_d on 2^22 random 64-bit patterns (its integer exponent extraction is defined for every one), positive normal
    doubles and the mantissa switch at sqrt 2; mis_round_d on |v| < 2^31 with the ties."""
    rng = np.random.default_rng(41)
    x = np.concatenate([rng.integers(0, 1 << 64, N_RANDOM, dtype=np.uint64).view(np.float64), np.exp2(rng.uniform(-1022.0, 1023.0, 1 << 20)),
                        math.sqrt(2.0) * (1.0 + rng.uniform(-1e-6, 1e-6, 1 << 16)), SPEC.astype(np.float64), [2.2250738585072014e-308, 5e-324]])
    _host_and_device(ctx, "log_d", x)
    k = rng.integers(-(1 << 31) + 1, (1 << 31) - 2, 1 << 18).astype(np.float64)
    bits = rng.integers(0, 1 << 64, 9 << 20, dtype=np.uint64).view(np.float64)
    with np.errstate(invalid="ignore"):
        bits = bits[np.abs(bits) < 2147483647.0][:N_RANDOM]
    assert bits.size == N_RANDOM
    v = np.concatenate([bits, rng.uniform(-2147483647.0, 2147483647.0, 1 << 21), rng.uniform(-70000.0, 70000.0, 1 << 20), k + 0.5, np.nextafter(k + 0.5, np.inf),
                        np.nextafter(k + 0.5, -np.inf), np.arange(-70000, 70000) + 0.5, [2147483647.0, -2147483647.0, 0.0, -0.0, 4.9e-324, 0.49999999999999994]])
    dev = _host_and_device(ctx, "round_d", v)
    assert np.array_equal(dev, np.rint(v).astype(np.int64))


def test_aid_refuses_more_than_2_20_elements_with_a_context(ctx):
    import ctypes as C
    from image_stitching_amd import _capi as capi
    x = np.zeros((1 << 20) + 1, F)
    rc = ctx.lib.mis_debug_math(ctx.h, capi.MATHX["sin"][0], x.ctypes.data_as(C.c_void_p), None, x.ctypes.data_as(C.c_void_p), x.size)
    assert rc != 0 and b"2^20" in ctx.lib.mis_last_error(ctx.h)
