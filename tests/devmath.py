"""Calls of the library's math test aids (mis_debug_math, mis_debug_math_f32) and float32 enumeration helpers, shared by
test_dev_math_cpu.py and test_dev_math_gpu.py.  ctx None: the host evaluation (libmistitch.so loads without a device)."""
import ctypes as C
import math

import numpy as np

F = np.float32

CHUNK = 1 << 20          # the aid's limit per call with a context (it stages through the context's grow-only scratch)
OLD = {"log": 0, "tan": 1, "sinh": 2, "asin": 3, "atan": 4, "exp": 5}        # mis_debug_math_f32's six


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def call(name, a, b=None, ctx=None):
    """out[i] = name(a[i][, b[i]]) through the aid; arrays of the dtypes the function has (capi.MATHX)."""
    from image_stitching_amd import _capi as capi
    lib = capi.load()
    if name in OLD:
        ta, tb, to = "f4", None, "f4"
    else:
        code, ta, tb, to = capi.MATHX[name]
    a = np.ascontiguousarray(a, ta).ravel()
    assert (b is not None) == (tb is not None), name
    if tb:
        b = np.ascontiguousarray(b, tb).ravel()
        assert b.size == a.size
    out = np.empty(a.size, to)
    step = CHUNK if ctx is not None else max(a.size, 1)
    for s in range(0, a.size, step):
        aa, oo = a[s:s + step], out[s:s + step]
        h = ctx.h if ctx is not None else None
        if name in OLD:
            rc = lib.mis_debug_math_f32(h, OLD[name], _ptr(aa), _ptr(oo), aa.size)
        else:
            rc = lib.mis_debug_math(h, code, _ptr(aa), _ptr(b[s:s + step]) if tb else None, _ptr(oo), aa.size)
        if ctx is not None:
            ctx.check(rc)
        assert rc == 0, (name, rc)
    return out


# ------------------------------------------------------------------------------------------------ float32 enumeration
def f2o(x):
    """float32 -> its index in the order of the reals (int64; +0 and -0 both 0): neighbours in value differ by 1."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u < 0x80000000, u, -(u & 0x7fffffff))


def o2f(o):
    o = np.asarray(o, np.int64)
    u = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return u.view(np.float32)


def every_nth(lo, hi, step, chunk=1 << 22):
    """Yields float32 arrays: every `step`-th float32 of [lo, hi] in increasing order (hi itself appended)."""
    a, b = int(f2o(np.float32(lo))), int(f2o(np.float32(hi)))
    for s in range(a, b + 1, step * chunk):
        yield o2f(np.arange(s, min(s + step * chunk, b + 1), step, dtype=np.int64))
    yield np.array([hi], np.float32)


def around(centres, ulps=4096):
    """Every float32 within `ulps` steps of each centre (rounded to float32 first), concatenated."""
    k = np.arange(-ulps, ulps + 1, dtype=np.int64)
    return np.concatenate([o2f(int(f2o(np.float32(c))) + k) for c in centres])


def random_bits(rng, n, keep=None):
    """n float32 with random bit patterns; `keep`: predicate on the array -> boolean mask of the function's domain (values outside
    are drawn again)."""
    out = np.empty(0, np.float32)
    while out.size < n:
        x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        if keep is not None:
            with np.errstate(invalid="ignore"):
                x = x[keep(x)]
        out = np.concatenate([out, x])
    return out[:n]


def same_bits(a, b):
    """Elementwise: equal in every bit, NaNs compared as NaNs."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype.kind != "f":
        return a == b
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(u) == b.view(u)))


# ------------------------------------------------------------------------------------------------ exact references and inputs
def fast_atan2_f32(y, x):
    """cv::fastAtan2 with every operation rounded to float32, in the written order."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    scale = F(180.0 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * scale, F(-0.3258083974640975) * scale, F(0.1555786518463281) * scale, F(-0.04432655554792128) * scale
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    with np.errstate(all="ignore"):
        c = np.where(first, ay / (ax + eps), ax / (ay + eps))
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
        a = np.where(first, a, F(90.0) - a)
        a = np.where(x < 0, F(180.0) - a, a)
        a = np.where(y < 0, F(360.0) - a, a)
    assert a.dtype == F
    return a


def fast_atan2_inputs(rng, n):
    """n random vectors over six decades, integer moments as ORB's intensity centroid has them, the axes, zeros and x == +-y."""
    m = rng.standard_normal((2, n)) * np.power(10.0, rng.uniform(-3.0, 3.0, n))
    k = rng.integers(-(1 << 22), 1 << 22, (2, 1 << 12)).astype(np.float64)
    d = np.power(10.0, rng.uniform(-30.0, 30.0, 1 << 10))
    ax = np.array([[0, 0], [0, 1], [1, 0], [0, -1], [-1, 0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [1e-45, 0], [0, 1e-45], [3e38, 3e38], [1e-30, -1e-30]]).T
    y = np.concatenate([m[0], k[0], d, -d, d, -d, ax[0]])
    x = np.concatenate([m[1], k[1], d, d, -d, -d, ax[1]])
    return y.astype(F), x.astype(F)


def ieee_inputs(rng, n):
    """float32 for the correctly-rounded operations: random bit patterns (every class of value), subnormals, the neighbourhood of
    the subnormal threshold, powers of two and their neighbours, values whose square root / quotient is subnormal or overflows."""
    tiny = F(1.1754944e-38)
    a = np.concatenate([random_bits(rng, n), around([tiny, -tiny, 0.0, 1.0, 4.0, 3.4028235e38, 2.0 ** -64, 2.0 ** 64], 1024),
                        np.exp2(np.arange(-149.0, 128.0)).astype(F), o2f(rng.integers(1, 1 << 23, 1 << 14)), -o2f(rng.integers(1, 1 << 23, 1 << 14)),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F)])
    return np.ascontiguousarray(a, F)


def ieee_pairs(rng, n):
    """(a, b) for a / b: random patterns against random patterns; quotients that are subnormal, that round across the threshold
    2^-126, that overflow, 0 / 0, x / 0, inf / inf and subnormal operands."""
    a = ieee_inputs(rng, n)
    b = np.ascontiguousarray(rng.permutation(ieee_inputs(rng, n))[: a.size], F)
    m = 1 << 16
    one = o2f(rng.integers(0x3f800000, 0x40000000, m))                                 # [1, 2)
    two = o2f(rng.integers(0x3f800000, 0x40000000, m))
    ea = rng.integers(-126, -100, m)
    eb = rng.integers(0, 40, m)                                                           # quotient about 2^-126 .. 2^-166
    xa = np.concatenate([np.ldexp(one, ea).astype(F), np.ldexp(one, rng.integers(100, 127, m)).astype(F), o2f(rng.integers(1, 1 << 23, m)),
                         np.array([0.0, 1.0, np.inf, -1.0, 0.0, np.nan, 1.0], F)])
    xb = np.concatenate([np.ldexp(two, eb).astype(F), np.ldexp(two, -rng.integers(0, 60, m)).astype(F), two,
                         np.array([0.0, 0.0, np.inf, -0.0, -0.0, 1.0, np.nan], F)])
    return np.concatenate([a, xa]), np.concatenate([b, xb])


def reflect_cases():
    """(p, len, BORDER_REFLECT_101 index, BORDER_REFLECT index) for len 1 .. 9 and p in [-3 len, 3 len]: the index maps that
    np.pad(mode="reflect") and np.pad(mode="symmetric") apply to arange(len)."""
    rows = []
    for n in range(1, 10):
        r101 = np.pad(np.arange(n), 3 * n + 1, mode="reflect")
        rsym = np.pad(np.arange(n), 3 * n + 1, mode="symmetric")
        for p in range(-3 * n, 3 * n + 1):
            rows.append((p, n, r101[p + 3 * n + 1], rsym[p + 3 * n + 1]))
    return np.array(rows, np.int32)
