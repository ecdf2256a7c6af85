"""Builds and drives tests/harness/ba_affine_host_harness.cpp, the host twin of the affine-partial bundle adjuster and the affine
estimator (shared by the CPU and the GPU test of refimpl_affine_family)."""
import ctypes as C
import os
import subprocess

import numpy as np

import refimpl_motion as rm
from ba_ray_twin import HIPCC, KP

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_dir):
    """-> the loaded harness, or None where hipcc is absent."""
    if not os.path.exists(HIPCC):
        return None
    so = os.path.join(str(tmp_dir), "libbaaffineharness.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-x", "hip",
                        os.path.join(HERE, "harness", "ba_affine_host_harness.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return C.CDLL(so)


def marshal_table(n, tab):
    """The n x n table of dicts as a MisMatchesInfo array -> (array, the numpy arrays that own its memory)."""
    from image_stitching_amd import _capi as capi
    keep = []
    mis = (capi.MisMatchesInfo * (n * n))()
    for k, m in enumerate(tab):
        mm = np.zeros(len(m["matches"]), rm.DMATCH_DTYPE)
        if len(mm):
            names = m["matches"].dtype.names
            mm["query_idx"], mm["train_idx"] = m["matches"][names[0]], m["matches"][names[1]]
        mk = np.ascontiguousarray(m["inliers_mask"], np.uint8) if m["inliers_mask"] is not None else np.zeros(0, np.uint8)
        keep += [mm, mk]
        mis[k].src_img_idx, mis[k].dst_img_idx, mis[k].n_matches = int(m["src_img_idx"]), int(m["dst_img_idx"]), len(mm)
        mis[k].matches = C.cast(mm.ctypes.data, C.POINTER(capi.MisDMatch)) if len(mm) else None
        mis[k].inliers_mask = C.cast(mk.ctypes.data, C.POINTER(C.c_uint8)) if len(mk) else None
        mis[k].num_inliers, mis[k].has_H, mis[k].confidence = int(m["num_inliers"]), 1 if m["has_H"] else 0, float(m["confidence"])
        if m["has_H"]:
            for q, v in enumerate(np.asarray(m["H"], np.float64).reshape(9)):
                mis[k].H[q] = v
    return mis, keep


def _cams_out(cams, n):
    return [dict(focal=cams[k].focal, aspect=cams[k].aspect, ppx=cams[k].ppx, ppy=cams[k].ppy, R=np.array(list(cams[k].R)).reshape(3, 3),
                 t=np.array(list(cams[k].t))) for k in range(n)]


def run(lib, n, xy, tab, start, thr, size=(rm.W, rm.H)):
    """-> (return code, cameras) of the twin's adjuster on host keypoints xy (list of (k, 2) float32) and the n x n table of dicts."""
    from image_stitching_amd import _capi as capi
    keep = []
    fa = (capi.MisFeatures * n)()
    for i, p in enumerate(xy):
        kp = np.zeros(len(p), KP)
        kp["x"], kp["y"] = p[:, 0], p[:, 1]
        keep.append(kp)
        fa[i].img_idx, fa[i].img_w, fa[i].img_h, fa[i].n = i, size[0], size[1], len(kp)
        fa[i].keypoints = kp.ctypes.data
    mis, k2 = marshal_table(n, tab)
    cams = (capi.MisCameraParams * n)()
    for k, c in enumerate(start):
        cams[k].focal, cams[k].aspect, cams[k].ppx, cams[k].ppy = c["focal"], c.get("aspect", 1.0), c["ppx"], c["ppy"]
        for q, v in enumerate(np.asarray(c["R"], np.float64).reshape(9)):
            cams[k].R[q] = v
        for q, v in enumerate(np.asarray(c.get("t", np.zeros(3)), np.float64).reshape(3)):
            cams[k].t[q] = v
    lib.dbg_bundle_adjust_affine_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    rc = lib.dbg_bundle_adjust_affine_partial(C.addressof(fa), C.addressof(mis), n, thr, C.addressof(cams))
    return rc, _cams_out(cams, n)


def estimate(lib, n, tab):
    """-> cameras of the twin's estimator on the n x n table of dicts."""
    from image_stitching_amd import _capi as capi
    mis, keep = marshal_table(n, tab)
    cams = (capi.MisCameraParams * n)()
    lib.dbg_estimate_affine_cameras.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert lib.dbg_estimate_affine_cameras(C.addressof(mis), n, C.addressof(cams)) == 0
    return _cams_out(cams, n)


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(rm._bits(x[k]), rm._bits(y[k])) for x, y in zip(a, b) for k in ("R", "focal", "aspect", "ppx", "ppy", "t"))
