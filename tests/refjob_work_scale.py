"""Test helper: main()'s sequence WITH a work scale, restated on the CPU from the oracle's stage functions.

oracle/job.py restates the sequence at work_megapix = -1 only.  This module follows the reference lines that a work scale
changes (image_stitching/image_stitching.cpp), stage by stage:

  :589-603    work_megapix < 0 -> work_scale = 1, the frame as it is; otherwise work_scale = min(1, sqrt(work_megapix * 1e6 / area))
              from the first frame and EVERY frame through resize(full, img, Size(), work_scale, work_scale, INTER_LINEAR_EXACT)
              (no |scale - 1| > 0.1 test)
  :613        features from the work image (features[i].img_size = the work size)
  :607, :619  seam_work_aspect = seam_scale / work_scale; the seam-scale image is resized from the FULL frame
  :635-637    cam.focal, ppx, ppy *= work_scale (double) before matching
  :661-726    pruning, bundle adjustment, wave correction: in work units
  :884-895    median focal of the kept (work-unit) cameras
  :1113-1125  compose_work_aspect = compose_scale / work_scale; warped_image_scale *= (float)compose_work_aspect; focal, ppx, ppy *=
              compose_work_aspect (double)
  :1129-1146  frames and sizes resized by compose_scale only when |compose_scale - 1| > 0.1

Written from those lines, not from the package under test.  Never imported by the product."""
import numpy as np

import oracle as o


def work_scale_of(work_megapix, w, h):
    """(:589-603) -> work_scale (double)"""
    if work_megapix < 0:
        return 1.0
    return min(1.0, float(np.sqrt(work_megapix * 1e6 / (w * h))))


def work_images(frames, work_scale):
    """(:602) every frame resized by factor; the frame itself only when work_megapix < 0 (a factor of exactly 1 is the identity of
    INTER_LINEAR_EXACT: checked by tests/test_work_scale_gpu.py against oracle.resize_exact)"""
    return [o.resize_exact(np.ascontiguousarray(f), fx=work_scale, fy=work_scale) if work_scale != 1.0 else np.ascontiguousarray(f) for f in frames]


def features_of(images, features_type="orb"):
    h, w = images[0].shape[:2]
    finder = o.Sift(w, h) if features_type == "sift" else o.Orb(w, h)
    feats = []
    for im in images:
        k, d = finder.run(im)
        feats.append(dict(img_w=w, img_h=h, kps=k, xy=np.stack([k["x"], k["y"]], 1), desc=d))
    return feats


def _median_focal(focals):
    focals = sorted(focals)
    k = len(focals)
    return float(np.float32(focals[k // 2])) if k % 2 == 1 else float(np.float32(focals[k // 2 - 1] + focals[k // 2]) * np.float32(0.5))


def stitch_job_work_scale(frames, cams, work_megapix, refine=False, seams=False, seam_megapix=0.1, compose_megapix=-1, conf_thresh=0.95, match_conf=0.32,
                          blend_type=o.BLEND_MULTI_BAND, blend_strength=5.0, ba_refine_mask="_____", wave_correct="horiz", block_size=64, nr_filtering=2,
                          features_type="orb"):
    """frames: (H, W, 3) uint8 arrays at full resolution; cams: dicts with K (full-resolution pixels) and R.
    refine: BundleAdjusterReproj + waveCorrect; seams: BlocksGainCompensator + DpSeamFinder(COLOR) at seam scale.
    -> dict(work_scale, work_size, features, matches, confidence, indices, cameras (work units, kept), scale, seam_masks, gain_maps,
    rois, pano, mask, num_bands, pano_size)."""
    n = len(frames)
    H, W = frames[0].shape[:2]
    ws = work_scale_of(work_megapix, W, H)
    wimgs = work_images(frames, ws)
    feats = features_of(wimgs, features_type)
    # :635-637, in double like CameraParams
    wcams = []
    for c in cams:
        K = np.asarray(c["K"], np.float64)
        focal = float(K[0, 0])
        wcams.append(dict(focal=focal * ws, aspect=float(K[1, 1]) / focal, ppx=float(K[0, 2]) * ws, ppy=float(K[1, 2]) * ws, R=np.asarray(c["R"], np.float64)))
    pm = o.match_all_pairs(feats, o.match_default_params(match_conf=match_conf))
    conf = np.array([m["confidence"] for m in pm], np.float64).reshape(n, n)
    indices = [int(i) for i in o.leave_biggest_component(conf, conf_thresh)]
    k = len(indices)
    kept = [dict(wcams[i]) for i in indices]
    if refine:
        sub = []
        for a, i in enumerate(indices):
            for b, j in enumerate(indices):
                m = dict(pm[i * n + j])
                m["src_img_idx"], m["dst_img_idx"] = a, b
                sub.append(m)
        kept, _ = o.bundle_adjust_reproj([feats[i] for i in indices], sub, kept, conf_thresh, ba_refine_mask)
        if wave_correct != "no":
            for c, R in zip(kept, o.wave_correct([c["R"] for c in kept], 1 if wave_correct == "vert" else 0)):
                c["R"] = R
    scale = _median_focal([c["focal"] for c in kept])

    def Kf(c, a=1.0):
        f = c["focal"] * a
        return np.array([[f, 0, c["ppx"] * a], [0, f * c.get("aspect", 1.0), c["ppy"] * a], [0, 0, 1]], np.float64).astype(np.float32)

    seam_masks, gain_maps, comp = None, None, None
    if seams:
        seam_scale = min(1.0, float(np.sqrt(seam_megapix * 1e6 / (W * H))))
        swa = np.float32(seam_scale / ws)                                           # :607, used as float at :980-983
        sscale = float(np.float32(np.float32(scale) * swa))                         # :973
        s_corners, s_imgs, s_masks = [], [], []
        for i, c in zip(indices, kept):
            f = np.ascontiguousarray(frames[i])
            img = o.resize_exact(f, fx=seam_scale, fy=seam_scale) if seam_scale < 1 else f      # :619, from the full frame
            K = Kf(c)
            K[0, 0] *= swa; K[0, 2] *= swa; K[1, 1] *= swa; K[1, 2] *= swa
            R = np.asarray(c["R"], np.float64).astype(np.float32)
            wi, tl = o.warp_spherical(img, sscale, K, R)
            wm, _ = o.warp_spherical(np.full(img.shape[:2], 255, np.uint8), sscale, K, R, o.INTER_NEAREST, o.BORDER_CONSTANT)
            s_corners.append(tl); s_imgs.append(wi); s_masks.append(wm)
        comp = o.Compensator(block_size, block_size, nr_filtering)
        comp.feed(s_corners, s_imgs, s_masks)
        seam_masks = o.dp_seams(s_imgs, s_corners, s_masks)
        gain_maps = [comp.gain_map(q).copy() for q in range(k)]
    # ---- compositing loop (:1105-1146) ----
    cs = min(1.0, float(np.sqrt(compose_megapix * 1e6 / (W * H)))) if compose_megapix > 0 else 1.0
    cwa = cs / ws                                                                   # :1113
    wscale = float(np.float32(scale) * np.float32(cwa))                             # :1116
    resized = abs(cs - 1) > 1e-1
    cw, ch = (int(round(W * cs)), int(round(H * cs))) if resized else (W, H)
    Ks = [Kf(c, cwa) for c in kept]                                                 # :1123-1125
    Rs = [np.asarray(c["R"], np.float64).astype(np.float32) for c in kept]
    rois = [o.warp_roi(wscale, cw, ch, K, R) for K, R in zip(Ks, Rs)]
    corners = [(r[0], r[1]) for r in rois]
    sizes = [(r[2], r[3]) for r in rois]
    x0 = min(c[0] for c in corners); y0 = min(c[1] for c in corners)
    x1 = max(c[0] + s[0] for c, s in zip(corners, sizes)); y1 = max(c[1] + s[1] for c, s in zip(corners, sizes))
    btype, bands, sharp = o.blend_config(blend_type, blend_strength, x1 - x0, y1 - y0)
    bl = o.Blender(btype, bands, sharp)
    bl.prepare(corners, sizes)
    for q, i in enumerate(indices):
        f = np.ascontiguousarray(frames[i])
        img = o.resize_exact(f, fx=cs, fy=cs) if resized else f
        wi, tl = o.warp_spherical(img, wscale, Ks[q], Rs[q])
        wm, _ = o.warp_spherical(np.full(img.shape[:2], 255, np.uint8), wscale, Ks[q], Rs[q], o.INTER_NEAREST, o.BORDER_CONSTANT)
        if seams:
            wi = comp.apply(q, wi)
            wm = o.seam_mask_apply(seam_masks[q], wm)
        bl.feed(wi.astype(np.int16), wm, tl)
    pano, mask = bl.blend()
    return {"work_scale": ws, "work_size": (wimgs[0].shape[1], wimgs[0].shape[0]), "features": feats, "matches": pm, "confidence": conf, "indices": indices,
            "cameras": kept, "scale": scale, "seam_masks": seam_masks, "gain_maps": gain_maps, "rois": rois, "pano": pano, "mask": mask,
            "num_bands": bl.num_bands, "pano_size": (x1 - x0, y1 - y0)}
