"""Independent reading of OpenCV's HomographyBasedEstimator: focalsFromHomography, estimateFocal and the
rotation chain along the maximum spanning tree, in float64 numpy.  Nothing from the library or from oracle/ is imported; the
tree is this module's own (stable sort of the has_H pairs by num_inliers, descending; Kruskal; centres by leaf distance).

THE FOCALS are the same correctly rounded IEEE double operations on both sides (+, -, *, /, sqrt in the order A.16 writes them;
the library is built without contraction), so every f0, f1, ok flag, every sqrt(f0 f1) candidate and the median are compared AS
BITS.  A focal that is not ok is 0 on both sides.

THE ROTATIONS are compared within a bound, because the two sides may associate the 3 x 3 products and cofactors differently.
Every bound of this module comes from one device, stated once here: `Err` carries a value v with a first-order bound e on
|v - exact| through the arithmetic (u = 2^-53):

    a + b:   e = e_a + e_b + u |a + b|              a * b:   e = |a| e_b + |b| e_a + u |a b|
    a / b:   e = (e_a + |a / b| e_b) / |b| + u |a / b|         sqrt a:  e = e_a / (2 sqrt a) + u sqrt a

i.e. the condition of every operation times its inputs' errors plus its own rounding.  A quotient over a small denominator or a
cancelling sum therefore widens the bound by exactly its condition number; nothing is picked by hand.  The two constants that
are not derived by the arithmetic itself:

    E_R = 8 u    entry-wise distance of a float64 rotation matrix of tests' scenes from an exactly orthonormal one: the entries are
                 sums of at most three products of sines and cosines, each correctly rounded to 1 u of values <= 1 (3 u for the
                 products of three, 2 u for the two additions, rounded up to a power of two with the libm sin / cos at < 1 ulp).
    x 2          wherever a bound is applied to the difference of two evaluations (library against this module, or the table's H
                 built by numpy against the Err evaluation): each side is within e of the exact value.

  exact tables   H(i, j) = K_j R_j^T R_i K_i^-1 pushed through Err from rotation entries with error E_R: the bound on each focal
                 (`exact_focal_bound`) and on each chained rotation entry (`estimate_cameras` with the H entries' errors) covers the
                 construction of H, the library's own evaluation and the conditioning of the closed forms.
  real tables    the same chain evaluated from the table's H and the (bit-equal) focal with input error 0: e bounds the evaluation
                 error of either side; the float32 values handed on then differ by at most 2 e plus one float32 ulp (where the
                 two doubles straddle a rounding boundary): `check_cameras`.

THE SCENES' CONDITIONS (asserted on this module's results alone): the median focal within 10 % of the true one, every tree
edge's relative rotation, projected on SO(3) by SVD, within 2 degrees of R_from^T R_to.
"""
import math

import numpy as np

U = 2.0 ** -53
E_R = 8 * U


# ------------------------------------------------------------------------------------------------ values with first-order bounds
class Err:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + U * abs(v))

    __radd__ = __add__

    def __neg__(self):
        return Err(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Err.of(o))

    def __rsub__(self, o):
        return Err.of(o) + (-self)

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        return Err(v, abs(self.v) * o.e + abs(o.v) * self.e + U * abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        v = self.v / o.v
        return Err(v, (self.e + abs(v) * o.e) / abs(o.v) + U * abs(v))

    def sqrt(self):
        v = math.sqrt(self.v)
        return Err(v, self.e / (2 * v) + U * v)


def _mat(a, e=0.0):
    a = np.asarray(a, np.float64).reshape(3, 3)
    return [[Err(a[i, j], e) for j in range(3)] for i in range(3)]


def _mul(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def _inv(a):
    """The adjugate over the determinant."""
    c = [[a[(j + 1) % 3][(i + 1) % 3] * a[(j + 2) % 3][(i + 2) % 3] - a[(j + 1) % 3][(i + 2) % 3] * a[(j + 2) % 3][(i + 1) % 3] for j in range(3)] for i in range(3)]
    det = a[0][0] * c[0][0] + a[0][1] * c[1][0] + a[0][2] * c[2][0]
    return [[c[i][j] / det for j in range(3)] for i in range(3)]


def _T(a):
    return [[a[j][i] for j in range(3)] for i in range(3)]


def _vals(a):
    return np.array([[x.v for x in r] for r in a])


def _errs(a):
    return np.array([[x.e for x in r] for r in a])


def _K(f, ppx=0.0, ppy=0.0, aspect=1.0):
    f = Err.of(f)
    return [[f, Err(0), Err(ppx)], [Err(0), f * aspect, Err(ppy)], [Err(0), Err(0), Err(1)]]


# ------------------------------------------------------------------------------------------------ focalsFromHomography
def _pick(d1, d2, v1, v2):
    """-> (f, ok) of one focal from its two closed forms; the operands are numpy float64 scalars (inf and NaN as IEEE has them)."""
    if v1 < v2:
        v1, v2 = v2, v1
    if v1 > 0 and v2 > 0:
        return float(np.sqrt(v1 if abs(d1) > abs(d2) else v2)), True
    if v1 > 0:
        return float(np.sqrt(v1)), True
    return 0.0, False


def focals_from_homography(H):
    """-> (f0, f1, f0_ok, f1_ok) as SURVEY A.16 writes them; IEEE double throughout."""
    h = [np.float64(v) for v in np.asarray(H, np.float64).reshape(9)]
    with np.errstate(all="ignore"):
        d1 = h[6] * h[7]
        d2 = (h[7] - h[6]) * (h[7] + h[6])
        v1 = -(h[0] * h[1] + h[3] * h[4]) / d1
        v2 = (h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / d2
        f1, ok1 = _pick(d1, d2, v1, v2)
        d1 = h[0] * h[3] + h[1] * h[4]
        d2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4]
        v1 = -h[2] * h[5] / d1
        v2 = (h[5] * h[5] - h[2] * h[2]) / d2
        f0, ok0 = _pick(d1, d2, v1, v2)
    return f0, f1, ok0, ok1


def focal_candidates(n, tab):
    """sqrt(f0 f1) of every ordered pair with has_H whose two focals are ok, in table order."""
    out = []
    for k in range(n * n):
        if not tab[k]["has_H"]:
            continue
        f0, f1, ok0, ok1 = focals_from_homography(tab[k]["H"])
        if ok0 and ok1:
            with np.errstate(all="ignore"):
                out.append(float(np.sqrt(np.float64(f0) * np.float64(f1))))
    return out


def estimate_focal(n, tab, sizes):
    """-> (focal of every camera, the candidates)."""
    cand = focal_candidates(n, tab)
    if cand and len(cand) >= n - 1:
        s = sorted(cand)
        m = len(s)
        f = s[m // 2] if m % 2 == 1 else float((np.float64(s[m // 2 - 1]) + np.float64(s[m // 2])) * np.float64(0.5))
    else:
        f = float(sum(w + h for w, h in sizes)) / n
    return f, cand


# ------------------------------------------------------------------------------------------------ the spanning tree
def spanning_tree(n, tab):
    """-> (centres ascending, adjacency lists in the order the edges were added, edge list)."""
    pairs = [(i, j) for i in range(n) for j in range(n) if tab[i * n + j]["has_H"]]
    pairs.sort(key=lambda p: -float(np.float32(tab[p[0] * n + p[1]]["num_inliers"])))          # Python's sort is stable
    comp = list(range(n))
    adj = [[] for _ in range(n)]
    edges = []
    for i, j in pairs:
        if comp[i] == comp[j]:
            continue
        ci, cj = comp[i], comp[j]
        comp = [ci if c == cj else c for c in comp]
        adj[i].append(j)
        adj[j].append(i)
        edges.append((i, j))
    leafs = [i for i in range(n) if len(adj[i]) == 1]
    far = [0] * n
    for leaf in leafs:
        dist = {leaf: 0}
        q = [leaf]
        for v in q:
            for w in adj[v]:
                if w not in dist:
                    dist[w] = dist[v] + 1
                    q.append(w)
        for v, d in dist.items():
            far[v] = max(far[v], d)
    mn = min(far)
    return [i for i in range(n) if far[i] == mn], adj, edges


def walk(n, tab):
    """The tree's edges as the breadth-first walk from the first centre meets them -> (centre, [(from, to)])."""
    centres, adj, _ = spanning_tree(n, tab)
    c = centres[0]
    seen, q, out = {c}, [c], []
    for v in q:
        for w in adj[v]:
            if w not in seen:
                seen.add(w)
                q.append(w)
                out.append((v, w))
    return c, out


# ------------------------------------------------------------------------------------------------ the estimator
def estimate_cameras(n, tab, sizes, h_err=None, f_err=0.0):
    """-> dict(focal, candidates, centre, edges, R: (n, 3, 3) float64 before the float32 rounding, e: (n, 3, 3) the bound on every
    entry of R, rel: {(from, to): R_rel}, cams: list of dicts as the library returns them).  h_err: {(i, j): (3, 3) bound on the
    entries of H(i, j)} for tables whose H is itself computed (default: the table's H is the input, error 0); f_err: the bound on
    the focal where R is compared with a truth that has another one (K^-1 and K then count as independent: an overestimate)."""
    f, cand = estimate_focal(n, tab, sizes)
    fK = Err(f, f_err)
    centre, edges = walk(n, tab)
    eye = [[Err(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    R = {centre: eye}
    rel = {}
    with np.errstate(all="ignore"):
        for a, b in edges:
            Hm = np.asarray(tab[a * n + b]["H"], np.float64).reshape(3, 3)
            He = np.zeros((3, 3)) if h_err is None else h_err[(a, b)]
            H = [[Err(Hm[i, j], He[i, j]) for j in range(3)] for i in range(3)]
            r = _mul(_mul(_inv(_K(fK)), _inv(H)), _K(fK))
            rel[(a, b)] = _vals(r)
            R[b] = _mul(R[a], r)
    Rv = np.stack([_vals(R.get(i, eye)) for i in range(n)])
    Re = np.stack([_errs(R.get(i, eye)) for i in range(n)])
    cams = [dict(focal=f, aspect=1.0, ppx=0.5 * sizes[i][0], ppy=0.5 * sizes[i][1], R=Rv[i].astype(np.float32).astype(np.float64), t=np.zeros(3)) for i in range(n)]
    return dict(focal=f, candidates=cand, centre=centre, edges=edges, R=Rv, e=Re, rel=rel, cams=cams)


def check_cameras(ref, got, sizes):
    """The library's cameras `got` (dicts focal, aspect, ppx, ppy, R, t) against this module's: focal as bits, the fixed fields
    exactly, every R entry a float32 value within 2 e + one float32 ulp of the reference's.  -> the largest |difference| / bound."""
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, ref["cams"])):
        assert np.float64(g["focal"]).view(np.uint64) == np.float64(w["focal"]).view(np.uint64), ("focal bits", i, g["focal"], w["focal"])
        assert (g["aspect"], g["ppx"], g["ppy"]) == (1.0, 0.5 * sizes[i][0], 0.5 * sizes[i][1]) and not np.asarray(g["t"]).any(), (i, g)
        G = np.asarray(g["R"], np.float64).reshape(3, 3)
        assert np.array_equal(G, G.astype(np.float32).astype(np.float64)), "a returned rotation is not made of float32 values"
        bound = 2 * ref["e"][i] + np.spacing(np.maximum(np.abs(G), np.abs(w["R"])).astype(np.float32)).astype(np.float64)
        d = np.abs(G - w["R"])
        assert (d <= bound).all(), ("rotation outside its bound", i, d.max(), bound.min())
        worst = max(worst, float((d / bound).max()))
    return worst


# ------------------------------------------------------------------------------------------------ exact tables
def rot(yaw, pitch, roll):
    """R = Ry(yaw) Rx(pitch) Rz(roll), degrees."""
    y, p, r = (math.radians(v) for v in (yaw, pitch, roll))
    Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def exact_H(fi, Ri, fj, Rj):
    """H(i, j) = K_j R_j^T R_i K_i^-1 with centred K = diag(f, f, 1), from rotation entries known to E_R -> (values by numpy,
    bound on every entry: twice the Err bound -- numpy's evaluation and Err's are each within it)."""
    He = _mul(_mul(_K(fj), _mul(_T(_mat(Rj, E_R)), _mat(Ri, E_R))), _inv(_K(fi)))
    Hv = np.diag([fj, fj, 1.0]) @ Rj.T @ Ri @ np.diag([1 / fi, 1 / fi, 1.0])
    assert (np.abs(Hv - _vals(He)) <= _errs(He)).all()
    return Hv, 2 * _errs(He)


def exact_table(focals, Rs, edges, weights=None):
    """The n x n table of the pairs `edges` (i < j) with exact homographies both ways -> (table, {(i, j): bound on H's entries})."""
    n = len(focals)
    empty = dict(matches=np.zeros(0, [("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")]), inliers_mask=np.zeros(0, np.uint8))
    tab = [dict(empty, src_img_idx=-1, dst_img_idx=-1, num_inliers=0, has_H=0, H=None, confidence=0.0) for _ in range(n * n)]
    herr = {}
    for e, (i, j) in enumerate(edges):
        for a, b in ((i, j), (j, i)):
            Hv, He = exact_H(focals[a], Rs[a], focals[b], Rs[b])
            herr[(a, b)] = He
            tab[a * n + b] = dict(empty, src_img_idx=a, dst_img_idx=b, num_inliers=(weights or {}).get((i, j), 100 + 7 * e), has_H=1, H=Hv, confidence=2.0)
    return tab, herr


def exact_focal_bound(H, He):
    """Bounds on (f0, f1) of focalsFromHomography for an H whose entries are known to He: both closed forms of each focal through
    Err; the larger of the two bounds, as rounding may decide which form is taken.  Twice: the library's evaluation and this one."""
    h = [Err(v, e) for v, e in zip(np.asarray(H).reshape(9), np.asarray(He).reshape(9))]
    f1 = [(-(h[0] * h[1] + h[3] * h[4]) / (h[6] * h[7])).sqrt(), ((h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / ((h[7] - h[6]) * (h[7] + h[6]))).sqrt()]
    f0 = [(-h[2] * h[5] / (h[0] * h[3] + h[1] * h[4])).sqrt(), ((h[5] * h[5] - h[2] * h[2]) / (h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4])).sqrt()]
    return 2 * max(x.e for x in f0), 2 * max(x.e for x in f1)


# ------------------------------------------------------------------------------------------------ the scenes' conditions
def project_so3(R):
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64))
    Q = u @ vt
    return -Q if np.linalg.det(Q) < 0 else Q


def angle_deg(A, B):
    """The angle of the rotation A^T B."""
    c = (np.trace(np.asarray(A).T @ np.asarray(B)) - 1) / 2
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def scene_conditions(ref, true_f, true_R):
    """The median focal within 10 % of the truth; every tree edge's relative rotation, projected on SO(3), within 2 degrees of
    R_from^T R_to.  -> (focal ratio, the edges' errors in degrees)."""
    ratio = ref["focal"] / true_f
    assert 0.9 <= ratio <= 1.1, ("the median focal is off the truth by more than 10 %", ref["focal"], true_f)
    errs = []
    for (a, b) in ref["edges"]:
        errs.append(angle_deg(np.asarray(true_R[a]).T @ np.asarray(true_R[b]), project_so3(ref["rel"][(a, b)])))
        assert errs[-1] <= 2.0, ("a tree edge's rotation is off the truth by more than 2 degrees", a, b, errs[-1])
    return ratio, errs


# scene name -> (width, height, number of frames, first yaw); hfov 60 degrees, yaw 12 i + first, pitch 2 ((i % 3) - 1), roll 1.2 ((i % 2) - 0.5)
SCENES = {"A": (640, 360, 5, -24.0), "B": (480, 270, 3, -12.0)}
_scene_cache = {}


def scene(name):
    """-> (width, height, cameras of synth.make_camera, rendered frames (H, W, 3) uint8 BGR); rendered once."""
    if name not in _scene_cache:
        import synth
        w, h, n, y0 = SCENES[name]
        cams = [synth.make_camera(w, h, 60.0, 12.0 * i + y0, 2.0 * ((i % 3) - 1), 1.2 * ((i % 2) - 0.5)) for i in range(n)]
        _scene_cache[name] = (w, h, cams, [np.ascontiguousarray(synth.render_frame(c)) for c in cams])
    return _scene_cache[name]


def table_of(pm):
    """A PairwiseMatches of the library -> the table of dicts this module reads."""
    return [dict(src_img_idx=m.src_img_idx, dst_img_idx=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers,
                 has_H=1 if m.H is not None else 0, H=m.H, confidence=m.confidence) for m in pm]
