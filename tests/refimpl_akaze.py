"""numpy reference of the AKAZE finder, steps 1 - 9 of SURVEY Appendix A.19, written from that definition (not from the library's
akaze_core.h).  Float64 by default.  Every step is a function of its inputs, so that a test can apply it to planes downloaded from
the library: rounding then never compounds from stage to stage.

Every arithmetic step takes `dt` (np.float64 or np.float32) and `alt`: alt=True evaluates the same sums in another order (taps
reversed, columns before rows, fluxes and cell samples backwards).  The difference between (float64, alt=False) and (float32,
alt=True) is what the tests' bands are measured from."""
import math

import numpy as np

TAU_MAX = 0.25
PLANES = ("Lt", "Lsmooth", "flow", "Lx", "Ly", "Ldet")


def params(**kw):
    p = dict(threshold=0.001, n_octaves=4, n_octave_layers=4, max_points=-1)
    p.update(kw)
    return p


def fround(x):
    """fRound(x) = (int)(x + 0.5f): truncation towards zero"""
    return np.trunc(np.asarray(x) + 0.5).astype(np.int64)


# ------------------------------------------------------------------------------------------------ step 1
def plan(w, h, n_octaves=4, n_octave_layers=4, **_):
    levels = []
    for o in range(n_octaves):
        lw, lh = int(w / 2 ** o), int(h / 2 ** o)
        if o > 0 and (lw < 80 or lh < 40):
            break
        for j in range(n_octave_layers):
            esigma = 1.6 * 2.0 ** (j / n_octave_layers + o)
            v = esigma * 1.5 / 2 ** o
            levels.append(dict(level=len(levels), octave=o, sublevel=j, w=lw, h=lh, esigma=esigma, sigma_size=int(np.rint(v)),       # rint: ties to even
                               etime=0.5 * esigma * esigma, ratio=float(2 ** o), radius=esigma * 1.5))
            levels[-1]["border"] = int(fround(10.0 * math.sqrt(2.0) * levels[-1]["sigma_size"]))
    return levels


# ------------------------------------------------------------------------------------------------ step 2
def fed_schedule(T):
    """-> (n, the n steps in reordered order)"""
    n = int(math.ceil(math.sqrt(3.0 * T / TAU_MAX + 0.25) - 0.5 - 1.0e-8) + 0.5)
    scale = 3.0 * T / (TAU_MAX * n * (n + 1))
    tau = [scale * TAU_MAX / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * n + 2)) ** 2) for k in range(n)]
    kappa, p = n // 2, n + 1
    while any(p % d == 0 for d in range(2, int(math.isqrt(p)) + 1)):
        p += 1
    order, k = [], 0
    while len(order) < n:
        idx = ((k + 1) * kappa) % p - 1
        if idx < n:
            order.append(idx)
        k += 1
    return n, np.array([tau[i] for i in order]), order


def level_schedule(levels, i):
    return fed_schedule(levels[i]["etime"] - levels[i - 1]["etime"])


# ------------------------------------------------------------------------------------------------ step 3
def gray01(bgr, dt=np.float64):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return (((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(dt) / dt(255))


def gauss_taps(sigma):
    n = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)))
    n += 1 - n % 2
    x = np.arange(n) - (n - 1) / 2
    v = np.exp(-0.5 * x * x / (sigma * sigma))
    return v / v.sum()


def _filter_axis(img, taps, axis, mode, dt, alt, offsets=None):
    """sum_k taps[k] * img[. + offsets[k]] along an axis; mode "edge" (replicate) or "reflect" (101)"""
    n = len(taps)
    offsets = list(range(-(n // 2), n // 2 + 1)) if offsets is None else offsets
    r = max(abs(o) for o in offsets)
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode=mode)
    acc = np.zeros(img.shape, dt)
    ks = range(n - 1, -1, -1) if alt else range(n)
    L = img.shape[axis]
    for k in ks:
        if taps[k] == 0:
            continue
        sl = [slice(None), slice(None)]
        sl[axis] = slice(r + offsets[k], r + offsets[k] + L)
        acc = acc + dt(taps[k]) * p[tuple(sl)]
    return acc


def gauss_blur(img, sigma, dt=np.float64, alt=False):
    t = gauss_taps(sigma) if dt is np.float64 else gauss_taps(sigma).astype(np.float32)
    img = img.astype(dt)
    first, second = (0, 1) if alt else (1, 0)      # rows (along x) first unless alt
    return _filter_axis(_filter_axis(img, t, first, "edge", dt, alt), t, second, "edge", dt, alt)


def scharr(L, dt=np.float64, alt=False):
    p = np.pad(L.astype(dt), 1, mode="reflect")
    c = lambda dy, dx: p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx]
    three, ten = dt(3), dt(10)
    if alt:
        lx = three * (c(1, 1) - c(1, -1)) + (ten * (c(0, 1) - c(0, -1)) + three * (c(-1, 1) - c(-1, -1)))
        ly = three * (c(1, 1) - c(-1, 1)) + (ten * (c(1, 0) - c(-1, 0)) + three * (c(1, -1) - c(-1, -1)))
    else:
        lx = three * (c(-1, 1) - c(-1, -1)) + ten * (c(0, 1) - c(0, -1)) + three * (c(1, 1) - c(1, -1))
        ly = three * (c(1, -1) - c(-1, -1)) + ten * (c(1, 0) - c(-1, 0)) + three * (c(1, 1) - c(-1, 1))
    return lx, ly


def gradient_magnitudes(Lsmooth0, dt=np.float64, alt=False):
    lx, ly = scharr(Lsmooth0, dt, alt)
    return np.sqrt(lx * lx + ly * ly)[1:-1, 1:-1]


def kcontrast(Lsmooth0, dt=np.float64, alt=False, nbins=300, perc=0.7):
    """-> (k, hmax, the non-zero magnitudes): the bin that the walk stops in, over nbins, times hmax"""
    m = gradient_magnitudes(Lsmooth0, dt, alt).ravel()
    hmax = m.max() if m.size else 0.0
    nz = m[m != 0]
    if not hmax > 0:
        return 0.03, float(hmax), nz
    bins = np.minimum(np.floor(dt(nbins) * (nz / hmax)).astype(np.int64), nbins - 1)
    hist = np.bincount(bins, minlength=nbins)
    nthreshold = int(dt(len(nz)) * dt(perc))
    nel, k = 0, 0
    while nel < nthreshold and k < nbins:
        nel += hist[k]
        k += 1
    if nel < nthreshold:
        return 0.03, float(hmax), nz
    return float(dt(hmax) * (dt(k) / dt(nbins))), float(hmax), nz


def kcontrast_bin_edge_distance(nz, hmax, nbins=300):
    """the smallest distance of a magnitude to a histogram bin edge, in units of the magnitude"""
    if not len(nz):
        return np.inf
    v = nz.astype(np.float64) / float(hmax) * nbins
    return float(np.min(np.abs(v - np.rint(v))) * float(hmax) / nbins)


def _area_weights(n_src, n_dst, dt):
    s = dt(n_src) / dt(n_dst)
    W = np.zeros((n_dst, n_src), dt)
    for d in range(n_dst):
        f0, f1 = dt(d) * s, min(dt(d + 1) * s, dt(n_src))
        i = int(math.floor(f0))
        while i < f1 and i < n_src:
            W[d, i] = min(dt(i + 1), f1) - max(dt(i), f0)
            i += 1
    return W


def area_downsample(L, w_new, h_new, dt=np.float64, alt=False):
    """INTER_AREA's definition: the mean over [x s, (x + 1) s) with fractional end weights, normalised by the weights' sum"""
    h, w = L.shape
    Wx, Wy = _area_weights(w, w_new, dt), _area_weights(h, h_new, dt)
    L = L.astype(dt)
    acc = (Wy @ L) @ Wx.T if alt else Wy @ (L @ Wx.T)
    return (acc / np.outer(Wy.sum(1), Wx.sum(1))).astype(dt)


def level_start(Lt_prev, prev, cur, dt=np.float64, alt=False):
    if prev["octave"] != cur["octave"]:
        return area_downsample(Lt_prev, cur["w"], cur["h"], dt, alt)
    return Lt_prev.astype(dt)


def level_k(k0, octave, dt=np.float64):
    k = dt(k0)
    for _ in range(octave):
        k = dt(0.75) * k
    return k


def flow(Lsmooth, k, dt=np.float64, alt=False):
    lx, ly = scharr(Lsmooth, dt, alt)
    k = dt(k)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dt(1) / (dt(1) + (lx * lx + ly * ly) / (k * k))


def fed_step(Lt, g, tau, dt=np.float64, alt=False):
    Lt, g = Lt.astype(dt), g.astype(dt)
    fx = (g[:, 1:] + g[:, :-1]) * (Lt[:, 1:] - Lt[:, :-1])      # flux between x and x + 1, seen from x
    fy = (g[1:, :] + g[:-1, :]) * (Lt[1:, :] - Lt[:-1, :])
    z = np.zeros_like(Lt)
    fr, fl, fd, fu = z.copy(), z.copy(), z.copy(), z.copy()
    fr[:, :-1] = fx; fl[:, 1:] = -fx; fd[:-1, :] = fy; fu[1:, :] = -fy
    s = (fu + fd) + (fl + fr) if alt else ((fr + fl) + fd) + fu
    return Lt + dt(0.5) * dt(tau) * s


def diffuse(start, g, taus, octave, dt=np.float64, alt=False):
    Lt = start.astype(dt)
    for t in taus:
        Lt = fed_step(Lt, g, dt(t) / dt(4 ** octave), dt, alt)
    return Lt


# ------------------------------------------------------------------------------------------------ step 4
def deriv(L, s, axis, dt=np.float64, alt=False):
    """the derivative along `axis` (1: x, 0: y) at scale s: [-1, 0 .., +1] along it, [norm, w norm, norm] across, reflect-101"""
    w = 10.0 / 3.0
    norm = 1.0 / (2.0 * s * (w + 2.0))
    if dt is np.float32:
        w32 = np.float32(10.0) / np.float32(3.0)
        norm = np.float32(1) / (np.float32(2) * np.float32(s) * (w32 + np.float32(2)))
        w = w32
    d = _filter_axis(L.astype(dt), [-1.0, 1.0], axis, "reflect", dt, alt, offsets=[-s, s])
    return _filter_axis(d, [norm, dt(w) * dt(norm), norm], 1 - axis, "reflect", dt, alt, offsets=[-s, 0, s])


def first_derivatives(Lsmooth, s, dt=np.float64, alt=False):
    return deriv(Lsmooth, s, 1, dt, alt), deriv(Lsmooth, s, 0, dt, alt)


def ldet(Lx, Ly, s, dt=np.float64, alt=False):
    lxx, lyy, lxy = deriv(Lx, s, 1, dt, alt), deriv(Ly, s, 0, dt, alt), deriv(Lx, s, 0, dt, alt)
    return (lxx * lyy - lxy * lxy) * dt(s ** 4)


# ------------------------------------------------------------------------------------------------ steps 5 - 7
YES, MAYBE, NO = 2, 1, 0


def _tri(margin, band):
    return YES if margin > band else (NO if margin < -band else MAYBE)


def level_candidates(Ldet, lv, threshold, band=0.0):
    """-> list of (y, x, response, YES | MAYBE): the margin of a pixel is the least of Ldet - threshold and Ldet - neighbour"""
    b, h, w = lv["border"], lv["h"], lv["w"]
    if w <= 2 * b or h <= 2 * b:
        return []
    L = Ldet.astype(np.float64)
    c = L[b:h - b, b:w - b]
    margin = c - float(threshold)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                margin = np.minimum(margin, c - L[b + dy:h - b + dy, b + dx:w - b + dx])
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(margin >= -band)
    return [(int(y) + b, int(x) + b, float(L[y + b, x + b]), _tri(margin[y, x], band)) for y, x in zip(ys, xs)]


def refine(Ldet, x, y, dt=np.float64, alt=False):
    L = Ldet[y - 1:y + 2, x - 1:x + 2].astype(dt)
    half, two, quarter = dt(0.5), dt(2), dt(0.25)
    Dx, Dy = half * (L[1, 2] - L[1, 0]), half * (L[2, 1] - L[0, 1])
    if alt:
        Dxx, Dyy = (L[1, 2] - two * L[1, 1]) + L[1, 0], (L[2, 1] - two * L[1, 1]) + L[0, 1]
        Dxy = quarter * ((L[2, 2] - L[0, 2]) + (L[0, 0] - L[2, 0]))
    else:
        Dxx, Dyy = L[1, 2] + L[1, 0] - two * L[1, 1], L[2, 1] + L[0, 1] - two * L[1, 1]
        Dxy = quarter * (L[2, 2] + L[0, 0] - L[0, 2] - L[2, 0])
    det = Dxx * Dyy - Dxy * Dxy
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = dt(Dy * Dxy - Dx * Dyy) / det
        dy = dt(Dx * Dxy - Dy * Dxx) / det
    return float(dx), float(dy)


def keypoints(Ldets, levels, threshold=0.001, max_points=-1, band=0.0, band_d=0.0, stats=None, **_):
    """Steps 5 - 7 on the given Ldet planes, in float64, with three-valued comparisons: a comparison that holds or fails by no more
    than the band is MAYBE.  -> list of dicts in (level, y, x) order with `state` YES (decided: every run must have it) or MAYBE."""
    cands = []
    for lv, L in zip(levels, Ldets):
        cands += [dict(level=lv["level"], y=y, x=x, resp=r, state=s) for (y, x, r, s) in level_candidates(L, lv, threshold, band)]
    by_level = {}
    for c in cands:
        by_level.setdefault(c["level"], []).append(c)
    arr = {l: np.array([[c["x"], c["y"], c["resp"], c["state"]] for c in cs], np.float64) for l, cs in by_level.items()}
    out = []
    for p in cands:
        lp = levels[p["level"]]
        dropped = NO
        for l in (p["level"] - 1, p["level"], p["level"] + 1):
            if l not in arr:
                continue
            A, r = arr[l], levels[l]["ratio"]
            d2 = (A[:, 0] * r - p["x"] * lp["ratio"]) ** 2 + (A[:, 1] * r - p["y"] * lp["ratio"]) ** 2
            rad2 = lp["radius"] ** 2
            near_yes, near_may = d2 <= rad2 * (1 - 1e-5), d2 <= rad2 * (1 + 1e-5)
            order_q = np.array([(l, int(a[1]), int(a[0])) < (p["level"], p["y"], p["x"]) for a in A])
            same = (l == p["level"]) & (A[:, 0] == p["x"]) & (A[:, 1] == p["y"])
            win_yes = ((A[:, 2] - p["resp"] > band) | ((A[:, 2] == p["resp"]) & order_q & (band == 0))) & ~same
            win_may = ((A[:, 2] - p["resp"] >= -band) if band > 0 else ((A[:, 2] > p["resp"]) | ((A[:, 2] == p["resp"]) & order_q))) & ~same
            if np.any(near_yes & win_yes & (A[:, 3] == YES)):
                dropped = YES
                break
            if np.any(near_may & win_may):
                dropped = MAYBE
        if stats is not None:
            stats["candidates"] = stats.get("candidates", 0) + 1
            stats["suppressed"] = stats.get("suppressed", 0) + (dropped == NO)
        if dropped == YES:
            continue
        state = YES if (p["state"] == YES and dropped == NO) else MAYBE
        dx, dy = refine(Ldets[p["level"]], p["x"], p["y"])
        m = max(abs(dx), abs(dy))
        if not m <= 1 + band_d:      # (NaN / inf: refused)
            continue
        if m > 1 - band_d:
            state = MAYBE
        r = lp["ratio"]
        out.append(dict(level=p["level"], y=p["y"], x=p["x"], dx=dx, dy=dy, state=state, pt=((p["x"] + dx) * r + 0.5 * (r - 1), (p["y"] + dy) * r + 0.5 * (r - 1)),
                        size=2 * lp["radius"], response=p["resp"], octave=lp["octave"], class_id=p["level"]))
    if max_points > 0:
        rank = sorted(range(len(out)), key=lambda i: (-out[i]["response"], i))
        kept, ahead_all, ahead_yes = [], 0, 0
        for i in rank:
            k = out[i]
            if ahead_yes >= max_points:
                break
            if ahead_all >= max_points:
                k["state"] = MAYBE
            kept.append(i)
            ahead_all += 1
            ahead_yes += k["state"] == YES
        out = [out[i] for i in sorted(kept)]
    return out


# ------------------------------------------------------------------------------------------------ step 8
def orientation(Lx, Ly, lv, pt, size, dt=np.float64, alt=False):
    """-> (angle in degrees, the relative gap between the best two windows' scores, the least distance of a sample's angle to an edge
    of a window, the least distance of a sample coordinate to a rounding tie)"""
    r = dt(lv["ratio"])
    xf, yf = dt(pt[0]) / r, dt(pt[1]) / r
    s = int(fround(dt(0.5) * dt(size) / r))
    ij = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]
    I, J = np.array([a for a, _ in ij]), np.array([b for _, b in ij])
    fx, fy = xf + (I * s).astype(dt), yf + (J * s).astype(dt)
    tie = float(min(np.min(np.abs((fx + 0.5) - np.rint(fx + 0.5))), np.min(np.abs((fy + 0.5) - np.rint(fy + 0.5)))))
    ix, iy = np.clip(fround(fx), 0, lv["w"] - 1), np.clip(fround(fy), 0, lv["h"] - 1)
    g = (np.exp(-(I * I + J * J).astype(dt) / dt(12.5)) / (dt(12.5) * dt(math.pi))).astype(dt)
    rx, ry = g * Lx[iy, ix].astype(dt), g * Ly[iy, ix].astype(dt)
    ang = np.arctan2(ry, rx)
    ang = np.where(ang < 0, ang + dt(2 * math.pi), ang)
    two_pi, third = dt(2 * math.pi), dt(math.pi / 3)
    scores, sums, edge = [], [], np.inf
    order = slice(None, None, -1) if alt else slice(None)
    for k in range(42):
        a1 = dt(0.15) * dt(k)
        a2 = a1 - dt(5 * math.pi / 3) if a1 + third > two_pi else a1 + third
        if a1 < a2:
            m = (a1 < ang) & (ang < a2)
        else:
            m = ((ang > 0) & (ang < a2)) | ((ang > a1) & (ang < two_pi))
        edge = min(edge, float(np.min(np.abs(ang - a1))), float(np.min(np.abs(ang - a2))))
        if dt is np.float64 and not alt:
            sx, sy = rx[m].sum(), ry[m].sum()
        else:
            sx, sy = dt(0), dt(0)
            for v, w_ in zip(rx[m][order], ry[m][order]):
                sx, sy = sx + v, sy + w_
        scores.append(float(sx * sx + sy * sy))
        sums.append((sx, sy))
    best = int(np.argmax(scores))      # the first of equal scores
    top = sorted(scores, reverse=True)
    gap = (top[0] - top[1]) / top[0] if top[0] > 0 else 0.0
    if not scores[best] > 0:
        return 0.0, gap, edge, tie
    a = math.atan2(float(sums[best][1]), float(sums[best][0]))
    a = a + 2 * math.pi if a < 0 else a
    deg = a * 180.0 / math.pi
    return (deg - 360.0 if deg >= 360.0 else deg), gap, edge, tie


# ------------------------------------------------------------------------------------------------ step 9
GRIDS = (10, 7, 5)


def cells():
    """the 29 cells as (step, i0, j0), grid by grid, i outer"""
    return [(st, i, j) for st in GRIDS for i in range(-10, 10, st) for j in range(-10, 10, st)]


def bit_pairs():
    """the 486 bits as (cell a, cell b, channel): grid, then channel, then a < b"""
    out, base = [], 0
    for st in GRIDS:
        n = len(range(-10, 10, st)) ** 2
        for ch in range(3):
            out += [(base + a, base + b, ch) for a in range(n) for b in range(a + 1, n)]
        base += n
    return out


def mldb_values(Lt, Lx, Ly, lv, pt, size, angle_deg, dt=np.float64, alt=False, tie_band=0.0):
    """-> (values (29, 3), lo, hi): the cell means of (Lt, rx', ry'); lo / hi bound them over both roundings of every sample
    coordinate that lies within tie_band of a rounding tie"""
    r = dt(lv["ratio"])
    xf, yf = dt(pt[0]) / r, dt(pt[1]) / r
    s = dt(int(fround(dt(0.5) * dt(size) / r)))
    a = dt(angle_deg) * dt(math.pi / 180)
    co, si = dt(math.cos(a)), dt(math.sin(a))
    vals, lo, hi = np.zeros((29, 3), dt), np.zeros((29, 3)), np.zeros((29, 3))
    Lt, Lx, Ly = Lt.astype(dt), Lx.astype(dt), Ly.astype(dt)
    for c, (st, i0, j0) in enumerate(cells()):
        K, Lq = np.meshgrid(np.arange(i0, i0 + st), np.arange(j0, j0 + st), indexing="ij")
        K, Lq = K.ravel().astype(dt), Lq.ravel().astype(dt)
        fx, fy = xf + (-Lq * si + K * co) * s, yf + (Lq * co + K * si) * s

        def sample(ix, iy):
            ix, iy = np.clip(ix, 0, lv["w"] - 1), np.clip(iy, 0, lv["h"] - 1)
            vx, vy = Lx[iy, ix], Ly[iy, ix]
            return np.stack([Lt[iy, ix], -vx * si + vy * co, vx * co + vy * si], 1)
        ix, iy = fround(fx), fround(fy)
        v = sample(ix, iy)
        if dt is np.float64 and not alt:
            acc = v.sum(0)
        else:
            acc = np.zeros(3, dt)
            for row in (v[::-1] if alt else v):
                acc = acc + row
        vals[c] = acc / dt(st * st)
        vmin, vmax = v.astype(np.float64), v.astype(np.float64)
        if tie_band > 0:
            tx = np.abs((fx + 0.5) - np.rint(fx + 0.5)) <= tie_band
            ty = np.abs((fy + 0.5) - np.rint(fy + 0.5)) <= tie_band
            if tx.any() or ty.any():
                ax = np.where(tx, np.rint(fx + 0.5).astype(np.int64) - 1, ix)      # the other side of the tie
                bx = np.where(tx, np.rint(fx + 0.5).astype(np.int64), ix)
                ay = np.where(ty, np.rint(fy + 0.5).astype(np.int64) - 1, iy)
                by = np.where(ty, np.rint(fy + 0.5).astype(np.int64), iy)
                alts = np.stack([sample(x_, y_) for x_ in (ax, bx) for y_ in (ay, by)]).astype(np.float64)
                vmin, vmax = alts.min(0), alts.max(0)
        lo[c], hi[c] = vmin.sum(0) / (st * st), vmax.sum(0) / (st * st)
    return vals, lo, hi


def mldb_bits(vals):
    return np.array([vals[a, ch] > vals[b, ch] for a, b, ch in bit_pairs()], bool)


def mldb_decided(lo, hi, band):
    """a bit is decided when the two cells' value ranges are further apart than the band"""
    return np.array([(lo[a, ch] - hi[b, ch] > band) or (lo[b, ch] - hi[a, ch] > band) for a, b, ch in bit_pairs()], bool)


def pack_bits(bits):
    """486 bits -> 61 bytes, LSB first"""
    b = np.zeros(61 * 8, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b.reshape(61, 8), axis=1, bitorder="little").ravel()


def unpack_bits(row):
    return np.unpackbits(np.asarray(row, np.uint8)[:, None], axis=1, bitorder="little").ravel()[:486].astype(bool)


# ------------------------------------------------------------------------------------------------ the whole finder
def scale_space(bgr, dt=np.float64, alt=False, **kw):
    """-> (levels, list of dicts with the six planes and `start`, k-contrast)"""
    p = params(**kw)
    h, w = bgr.shape[:2]
    levels = plan(w, h, p["n_octaves"], p["n_octave_layers"])
    out = []
    img = gray01(bgr, dt)
    k0 = None
    for i, lv in enumerate(levels):
        if i == 0:
            ls = gauss_blur(img, 1.6, dt, alt)
            lt = ls
            k0 = kcontrast(ls, dt, alt)[0]
            g = flow(ls, level_k(k0, 0, dt), dt, alt)
        else:
            start = level_start(out[-1]["Lt"], levels[i - 1], lv, dt, alt)
            ls = gauss_blur(start, 1.0, dt, alt)
            g = flow(ls, level_k(k0, lv["octave"], dt), dt, alt)
            lt = diffuse(start, g, level_schedule(levels, i)[1], lv["octave"], dt, alt)
        lx, ly = first_derivatives(ls, lv["sigma_size"], dt, alt)
        out.append(dict(Lt=lt, Lsmooth=ls, flow=g, Lx=lx, Ly=ly, Ldet=ldet(lx, ly, lv["sigma_size"], dt, alt)))
    return levels, out, k0


def describe(levels, planes, kps, dt=np.float64, alt=False, tie_band=0.0):
    """orientation and MLDB of keypoints() output on the given planes: fills angle, gap, edge, tie, vals, lo, hi, desc"""
    for k in kps:
        lv, P = levels[k["level"]], planes[k["level"]]
        k["angle"], k["gap"], k["edge"], k["tie"] = orientation(P["Lx"], P["Ly"], lv, k["pt"], k["size"], dt, alt)
        k["vals"], k["lo"], k["hi"] = mldb_values(P["Lt"], P["Lx"], P["Ly"], lv, k["pt"], k["size"], k["angle"], dt, alt, tie_band)
        k["desc"] = pack_bits(mldb_bits(k["vals"]))
    return kps


def detect(bgr, dt=np.float64, alt=False, band=0.0, band_d=0.0, tie_band=0.0, **kw):
    p = params(**kw)
    levels, planes, k0 = scale_space(bgr, dt, alt, **p)
    kps = keypoints([P["Ldet"] for P in planes], levels, dt(p["threshold"]) if dt is np.float32 else np.float32(p["threshold"]), p["max_points"], band, band_d)
    return levels, planes, k0, describe(levels, planes, kps, dt, alt, tie_band)
