"""Independent reading of BundleAdjusterRay (ba_cost_func = "ray"), in float64 numpy.  Imports the
scenes, the tree's centre, the projection helpers and the constants of refimpl_motion; nothing from the library or from oracle/.

The library (csrc/motion_ray.hip, csrc/ba_ray.h, csrc/ba_ray_solve.h) restates OpenCV's adjuster step by step: a CvLevMarq state
machine over (focal, rotation VECTOR) per camera, a central-difference Jacobian with step 1e-3, normal equations solved by a
Jacobi SVD.  This module never iterates that way.  It holds

  the cost          S(p) = sum f_i f_j || ray_i - ray_j ||^2  over the pairs i < j with confidence > float32(conf_thresh) and the
                    matches whose mask byte is non-zero (query_idx -> image i, train_idx -> image j):
                    ray_c = R_c K_c^-1 (x, y, 1) normalised,  K_c = [[f_c, 0, W / 2], [0, f_c, H / 2], [0, 0, 1]]  with W, H the
                    FEATURES' image size: ppx, ppy and aspect of a camera are not read.  The residual of a match is the 3-vector
                    r = sqrt(f_i f_j) (ray_i - ray_j).
  the minimiser     p* of S, found as refimpl_motion.reference_ba finds its own: a damped Gauss-Newton on the rotation MANIFOLD
                    (R_c <- R_c exp([w]x)), ANALYTIC Jacobian, least squares on column-scaled J.  Gauge: S sees R_j^T R_i only,
                    so one rotation per connected component of the edge graph is held (the tree's centre where it lies in the
                    component, else the lowest index); the focal length of every camera that has an edge is free; a camera
                    without an edge is held entirely.  The same STATIONARITY TEST: the Gauss-Newton predicted decrease
                    g^T (J^T J)^+ g is at most `slack`, the evaluation noise of S.
                    S -> 0 as all focal lengths -> 0: there is no global minimum worth the name, both sides find the LOCAL
                    minimum reached from the scene's start, and `reference_ba_ray` asserts that its focal lengths stay within a
                    factor 2 of the start's (a sanity condition on the reference, not a tolerance on the library).

WHAT IS ASSERTED OF A RESULT p (`check_ba_ray`), assertions 1. - 4. of refimpl_motion's docstring carried over:
 1. ppx, ppy, aspect of every camera, and the focal length of a camera without an edge: the input's bits.
 2. the centre index (the camera whose returned R is the identity) and |R_c - I| <= U_OUT + 2^-30: the normalisation is the
    reprojection adjuster's, same derivation.
 3. S* - slack <= S(p) <= S* + E, S(p) on the returned focal lengths and the returned rotations PROJECTED on SO(3), and
    |R^T R - I| <= ORTHO_BAND for every returned R.
    Output model as there: R_i^out = fl32(M fl32(R_i)), M = fl32(R_c^-1).  This cost is invariant under a common ORTHOGONAL left
    factor only (the rays are normalised after the rotation), so the projection is not a convenience here: M = O (I + e), e
    symmetric of size 4 u, M R_i = (O R_i)(I + R_i^T e R_i) is in polar form, projecting returns the common factor O and the
    tangent part of the entry roundings.  Every one of the 9 n output entries is off by at most u_k = U_OUT = (sqrt 3 + 3) 2^-24
    (same three terms).  First order,  || r(p) - r(p^) || <= sum_k u_k || dr / dR_k || =: sqrt E,  the columns taken over all
    residuals at the re-gauged minimiser Q*_i = R_c*^T R_i*; with ray = R v / |R v|, v the unit vector of K^-1 x,
    d ray / dR[a, b] = (I - ray ray^T) e_a v_b, and dr / dR_i[a, b] = +- sqrt(f_i f_j) of that (+ for the edge's first camera).
    At the minimiser the residual is orthogonal to every tangent column, so a result that sits at the minimiser exceeds S* by the
    square only:  E = (sum_k u_k || dr / dR_k ||)^2.  The focal lengths leave as the solver's doubles: no rounding term.
    slack: a residual component is sqrt(f_i f_j) times a difference of two unit-vector components; each side is about 30 double
    roundings on magnitudes <= 1 (R K^-1: 9; H x: 5 each on values <= 1.2; the norm and the division), so
    e_r = 64 2^-52 max_c f_c bounds the evaluation error of a component, and S moves by at most 2 |r|_1 e_r + N e_r^2
    (N residual components).  As in refimpl_motion the returned `slack` is twice that (both sides evaluate).
    The yardstick Y = S(round(p*)) - S*: the same output rounding and projection applied to the reference's own minimiser.
 4. parameters, where the column-normalised gauge-fixed J at p* has condition number <= COND_CAP:
    |d_k| <= sqrt(E [(J^T J)^-1]_kk); rotations in the gauge of the reference, + ROT_ROUND for the output rounding of the two
    matrices compared (refimpl_motion 4.).  The focal lengths carry no rounding allowance.
    On the scenes of the case list E is 4e-5 .. 1.2e-2 and the focal bound 0.025 .. 0.14 px.  A central difference is exact in the
    gradient's zero only up to its truncation, but the LM step is J^T err with the TRUE err: its fixed point is the zero of
    J_num^T r, off the minimiser by (J^T J)^-1 (J_num - J)^T r, second order in the step 1e-3 times the residual; if that ever
    exceeded the bound the case would fail, not the bound move.
 5. refused input is the callers' business.

NOT PINNED here, because a fixed point cannot see them: the order of the sums of J^T J (the GPU test pins the device against the
host twin bit for bit instead), CvLevMarq's lambda schedule, the 1e-3 step.
"""
import math

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import refimpl_motion as rm
from refimpl_motion import COND_CAP, ORTHO_BAND, ROT_ROUND, THR, U24, U_OUT, H, W, _bits, _expm, _logm, _observations, f32, get_scene, make_scene, project_so3, projected, table, tree_centre

assert U24 == 2.0 ** -24
FIXED = ("ppx", "ppy", "aspect")


# ------------------------------------------------------------------------------------------------ the cost and its derivatives
def _unit(c, x, size):
    """v = K^-1 (x, y, 1) normalised, K from the image size; also |K^-1 x| and a = x - W/2, b = y - H/2."""
    a, b = x[:, 0] - size[0] * 0.5, x[:, 1] - size[1] * 0.5
    d = np.stack([a / c["focal"], b / c["focal"], np.ones(len(x))], 1)
    nd = np.linalg.norm(d, axis=1)
    return d / nd[:, None], nd, a, b


def _rays(c, x, size):
    """Unit rays R K^-1 x / |R K^-1 x| (R as given: the returned rotations are float32 values, not exactly orthonormal)."""
    v, _, _, _ = _unit(c, x, size)
    q = v @ np.asarray(c["R"], np.float64).T
    return q / np.linalg.norm(q, axis=1)[:, None]


def residuals(cams, obs, size=(W, H)):
    out = []
    for i, j, x1, x2 in obs:
        out.append((math.sqrt(cams[i]["focal"] * cams[j]["focal"]) * (_rays(cams[i], x1, size) - _rays(cams[j], x2, size))).reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


def cost(cams, obs, size=(W, H)):
    r = residuals(cams, obs, size)
    return float(r @ r)


def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def _side(c, x, size):
    """Of one camera's side of an edge (R orthonormal): the rays u = R v, du/df (m, 3), du/dw (m, 3, 3) for R <- R exp([w]x)."""
    v, nd, a, b = _unit(c, x, size)
    R = np.asarray(c["R"], np.float64)
    dd = np.stack([-a / c["focal"] ** 2, -b / c["focal"] ** 2, np.zeros(len(x))], 1)
    dv = (dd - v * np.sum(v * dd, 1)[:, None]) / nd[:, None]                  # (I - v v^T) dd / |d|
    return v @ R.T, dv @ R.T, -np.einsum("ab,nbc->nac", R, _skew(v)), v


def jacobian(cams, obs, free, size=(W, H)):
    """Analytic J (3 N x len(free)); free: list of (camera, name), name "focal" or "w0", "w1", "w2"."""
    col = {k: q for q, k in enumerate(free)}
    N = sum(len(o[2]) for o in obs)
    J = np.zeros((3 * N, len(free)))
    row = 0
    for i, j, x1, x2 in obs:
        m = len(x1)
        fi, fj = cams[i]["focal"], cams[j]["focal"]
        mult = math.sqrt(fi * fj)
        u1, du1f, du1w, _ = _side(cams[i], x1, size)
        u2, du2f, du2w, _ = _side(cams[j], x2, size)
        blk = {(i, "focal"): mult / (2 * fi) * (u1 - u2) + mult * du1f, (j, "focal"): mult / (2 * fj) * (u1 - u2) - mult * du2f}
        for k in range(3):
            blk[(i, "w%d" % k)] = mult * du1w[:, :, k]
            blk[(j, "w%d" % k)] = -mult * du2w[:, :, k]
        for key, b in blk.items():
            if key in col:
                J[row:row + 3 * m, col[key]] = np.asarray(b).reshape(-1)
        row += 3 * m
    return J


def rotation_entry_norms(cams, obs, size=(W, H)):
    """|| dr / dR_c[a, b] || over all residuals, (n, 3, 3):  dr = +- sqrt(f_i f_j) (I - u u^T) e_a v_b."""
    cols = {}
    for i, j, x1, x2 in obs:
        mult = math.sqrt(cams[i]["focal"] * cams[j]["focal"])
        for cam, x in ((i, x1), (j, x2)):
            u, _, _, v = _side(cams[cam], x, size)
            for a in range(3):
                ea = np.zeros(3)
                ea[a] = 1.0
                proj = ea[None, :] - u * u[:, a][:, None]                     # (I - u u^T) e_a, per observation
                for b in range(3):
                    cols.setdefault((cam, a, b), []).append((mult * proj * v[:, b][:, None]).reshape(-1))
    sq = np.zeros((len(cams), 3, 3))
    for (cam, a, b), parts in cols.items():
        vv = np.concatenate(parts)
        sq[cam, a, b] = vv @ vv
    return np.sqrt(sq)


# ------------------------------------------------------------------------------------------------ the minimiser
def reference_ba_ray(scene, tab, conf_thresh, start=None, size=(W, H)):
    """-> dict with p* (cams), S*, slack, E, Y, centre, free parameter list, the bound of every free parameter, cond, obs."""
    n, xy = scene["n"], scene["xy"]
    start = start or scene["start"]
    obs = _observations(n, xy, tab, conf_thresh)
    if sum(len(o[2]) for o in obs) == 0:
        return None
    obs = [o for o in obs if len(o[2])]                  # an edge without observations constrains nothing: its cameras are not 'in an edge'
    centre, _ = tree_centre(n, tab)
    adj = np.zeros((n, n))
    for i, j, _, _ in obs:
        adj[i, j] = 1
    _, lab = connected_components(csr_matrix(adj), directed=False)
    in_edge = sorted({c for o in obs for c in o[:2]})
    anchor = {}
    for c in in_edge:
        anchor.setdefault(lab[c], c)
    if centre in in_edge:
        anchor[lab[centre]] = centre
    free = []
    for c in in_edge:
        free.append((c, "focal"))
        if anchor[lab[c]] != c:
            free += [(c, "w0"), (c, "w1"), (c, "w2")]
    cams = [dict(focal=float(c["focal"]), aspect=float(c["aspect"]), ppx=float(c["ppx"]), ppy=float(c["ppy"]), R=project_so3(c["R"])) for c in start]

    def stepped(cs, delta):
        out = [dict(c) for c in cs]
        for q, (c, k) in enumerate(free):
            if k == "focal":
                out[c]["focal"] = cs[c]["focal"] + delta[q]
            elif k == "w0":
                out[c]["R"] = cs[c]["R"] @ _expm(delta[q:q + 3])
        return out

    def gn(cs, lam):
        r = residuals(cs, obs, size)
        J = jacobian(cs, obs, free, size)
        s = np.linalg.norm(J, axis=0)
        s[s == 0] = 1.0
        Js = J / s
        A = np.vstack([Js, math.sqrt(lam) * np.eye(len(free))]) if lam else Js
        b = np.r_[-r, np.zeros(len(free))] if lam else -r
        d = np.linalg.lstsq(A, b, rcond=1e-13)[0]
        d0 = d if not lam else np.linalg.lstsq(Js, -r, rcond=1e-13)[0]
        return d / s, float((Js @ d0) @ (Js @ d0)), r

    lam, S = 1e-3, cost(cams, obs, size)
    slack = pred = None
    for it in range(400):
        d, pred, r = gn(cams, lam)
        e_r = 64 * 2.0 ** -52 * max(c["focal"] for c in cams)
        slack = 2 * np.abs(r).sum() * e_r + len(r) * e_r ** 2
        if pred <= slack:
            break
        trial = stepped(cams, d)
        St = cost(trial, obs, size)
        if St < S and all(t["focal"] > 0 for t in trial):
            cams, S, lam = trial, St, (lam * 0.1 if lam > 1e-12 else 0.0)
        else:
            lam = max(lam, 1e-9) * 10
    assert pred <= slack, ("the reference did not reach its stationarity test", scene["name"], pred, slack, S)
    for c, s0 in zip(cams, start):
        assert 0.5 * s0["focal"] <= c["focal"] <= 2.0 * s0["focal"], ("the reference left the start's basin", scene["name"], c["focal"], s0["focal"])
    Rc = cams[centre]["R"]
    out = [dict(c, R=Rc.T @ c["R"]) for c in cams]
    S = cost(out, obs, size)
    E = float((U_OUT * rotation_entry_norms(out, obs, size).sum()) ** 2)
    rounded = [dict(c, R=f32(f32(np.linalg.inv(f32(cams[centre]["R"]))) @ f32(c["R"]))) for c in cams]
    Y = cost(projected(rounded), obs, size) - S
    Y_raw = cost(rounded, obs, size) - S
    J = jacobian(cams, obs, free, size)
    s = np.linalg.norm(J, axis=0)
    s[s == 0] = 1.0
    sv = np.linalg.svd(J / s, compute_uv=False)
    cond = float(sv[0] / sv[-1]) if sv[-1] > 0 else float("inf")
    bound = None
    if cond <= COND_CAP:
        cov = np.linalg.inv((J / s).T @ (J / s)) / np.outer(s, s)
        bound = np.sqrt(E * np.diag(cov))
    return dict(cams=cams, out=out, S=S, slack=2 * slack, E=E, Y=Y, Y_raw=Y_raw, centre=centre, free=free, bound=bound, cond=cond, obs=obs, anchor=anchor, lab=lab,
                in_edge=in_edge, start=start, size=size, n_obs=sum(len(o[2]) for o in obs))


def check_ba_ray(ref, got, eligible):
    """The assertions 1. - 4. of the module docstring on a result `got` (list of dicts focal, aspect, ppx, ppy, R).
    -> dict(excess, over_Y, over_E, par_ratio, ...)."""
    start, size = ref["start"], ref["size"]
    for c in range(len(got)):
        for k in FIXED + (() if c in ref["in_edge"] else ("focal",)):
            assert np.array_equal(_bits(got[c][k]), _bits(float(start[c][k]))), ("held parameter moved", c, k, got[c][k], start[c][k])
    dev = [float(np.abs(np.asarray(g["R"]) - np.eye(3)).max()) for g in got]
    assert int(np.argmin(dev)) == ref["centre"] and dev[ref["centre"]] <= U_OUT + 2.0 ** -30, ("centre", ref["centre"], dev)
    for g in got:
        assert np.array_equal(np.asarray(g["R"]), f32(g["R"])), "a returned rotation is not made of float32 values"
        G = np.asarray(g["R"], np.float64)
        assert np.abs(G.T @ G - np.eye(3)).max() <= ORTHO_BAND, ("a returned rotation is not orthonormal within its band", np.abs(G.T @ G - np.eye(3)).max())
    S = cost(projected(got), ref["obs"], size)
    excess = S - ref["S"]
    res = dict(excess=excess, over_Y=excess / ref["Y"] if ref["Y"] else float("nan"), over_E=excess / ref["E"], par_ratio=None,
               raw_excess=cost(got, ref["obs"], size) - ref["S"], Y=ref["Y"], Y_raw=ref["Y_raw"], E=ref["E"], cond=ref["cond"], S=ref["S"])
    assert -ref["slack"] <= excess <= ref["E"], ("cost", S, ref["S"], excess, ref["slack"], ref["E"])
    assert eligible == (ref["cond"] <= COND_CAP), ("the case list names this case %s, its condition number is %.3g" % ("eligible" if eligible else "cost only", ref["cond"]))
    if eligible:
        worst = 0.0
        for q, (c, k) in enumerate(ref["free"]):
            if k == "focal":
                ratio = abs(got[c][k] - ref["cams"][c][k]) / ref["bound"][q]
            elif k == "w0":
                a = ref["anchor"][ref["lab"][c]]
                Qs = ref["cams"][a]["R"].T @ ref["cams"][c]["R"]
                Qg = project_so3(np.linalg.inv(np.asarray(got[a]["R"])) @ np.asarray(got[c]["R"]))
                d = _logm(Qs.T @ Qg)
                ratio = max(abs(d[t]) / (ref["bound"][q + t] + ROT_ROUND) for t in range(3))
            else:
                continue
            assert ratio <= 1.0, ("parameter outside its bound", c, k, ratio)
            worst = max(worst, ratio)
        res["par_ratio"] = worst
    return res


# ------------------------------------------------------------------------------------------------ the case list
_EXTRA = {
    # the edge (0, 2) keeps exactly one inlier: mask 1 on its first match, 0 on the others (the list is as long as `pts`)
    "chain5-one": lambda: make_scene("chain5-one", rm._chain(5), rm._chain_edges(5), 0.3, 4, mask_bytes={(0, 2): [1] + [0] * 59}),
    # more than 512 observations on an edge: every workgroup and chunk boundary of both kernels
    "big3": lambda: make_scene("big3", rm._chain(3), [(0, 1), (1, 2)], 0.3, 18, pts=900),
}
_cache = {}


def get_ray_scene(name):
    if name in _EXTRA:
        if name not in _cache:
            _cache[name] = _EXTRA[name]()
        return _cache[name]
    return get_scene(name)


def shifted_start(scene):
    """The scene's start with ppx, ppy 40 px off and aspect 1.1: the ray adjuster reads none of them."""
    return [dict(c, ppx=c["ppx"] + 40.0, ppy=c["ppy"] - 40.0, aspect=1.1) for c in scene["start"]]


# (scene, eligible): the reference's condition number decides, and check_ba_ray asserts the flag against it
RAY_CASES = [(name, True) for name in ("pair", "iso3", "chain5-s0", "chain5", "chain5-s1", "loop8", "two-comp", "zero-edge", "mask-mix", "conf-equal", "no-H",
                                       "star", "centre-off", "even-path", "scaled-R", "neg-det", "chain17", "chain5-one", "big3")]
_ref_cache = {}


def get_ray_reference(name):
    if name not in _ref_cache:
        s = get_ray_scene(name)
        _ref_cache[name] = reference_ba_ray(s, table(s), THR)
    return _ref_cache[name]
