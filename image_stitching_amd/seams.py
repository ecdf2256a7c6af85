"""The seam-scale step: cv::detail::ExposureCompensator's family and the seam finders (image_stitching.cpp:1002-1065, :1162-1171)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import Handle, _images, _points, as_image, torch
from .imgops import seam_mask_apply


def _seam_args(corners, images, masks):
    """The (corners, images, masks, n) arguments of the compensator's and the seam finders' entries."""
    return _points(corners), _images(images), _images(masks), len(masks)


class _Compensator(Handle):
    """One member of cv::detail::ExposureCompensator's family over mis_compensator_*.  feed() takes the seam-scale warped images /
    masks and their corners and never alters them, whatever nr_feeds is (the library works on private device copies); apply()
    multiplies an 8UC3 (or the fused warp's 16SC3) image by the gains, in place."""
    TYPE = None
    DESTROY = "mis_compensator_destroy"

    def _create(self, ctx, nr_feeds, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2):
        self.ctx = ctx
        h = C.c_void_p()
        params = capi.MisCompensatorParams(self.TYPE, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)
        ctx.check(ctx.lib.mis_compensator_create_ex(ctx.h, C.byref(params), C.byref(h)))
        self.h = h

    def feed(self, corners, images, masks):
        self.ctx.check(self.ctx.lib.mis_compensator_feed(self.h, *_seam_args(corners, images, masks)))

    def gains(self, index):
        """The accumulated gains of one image as three float64 (B, G, R; GainCompensator: the gain three times); the block types
        have a gain map instead and raise."""
        g = (C.c_double * 3)()
        self.ctx.check(self.ctx.lib.mis_compensator_gains(self.h, index, g))
        return np.array(g[:], np.float64)

    def gain_map(self, index):
        """The smoothed float32 gain map of one image: (by, bx) for BlocksGainCompensator, (by, bx, 3) for BlocksChannelsCompensator;
        GainCompensator and ChannelsCompensator have per-image gains instead and raise."""
        bx, by, ch = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.mis_compensator_gain_map_channels(self.h, index, None, 0, C.byref(bx), C.byref(by), C.byref(ch)))
        out = np.zeros((by.value, bx.value) if ch.value == 1 else (by.value, bx.value, ch.value), np.float32)
        self.ctx.check(self.ctx.lib.mis_compensator_gain_map_channels(self.h, index, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None, None, None))
        return out

    def debug_stats(self, i, j, channel=0):
        """Test hook (GainCompensator, ChannelsCompensator): (N_ij, I_ij, I_ji) of the last feed."""
        n, a, b = C.c_int(), C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.mis_compensator_debug_stats(self.h, i, j, channel, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def apply(self, index, corner, image, mask=None):
        """corner and mask are accepted for signature parity (OpenCV ignores them too)."""
        img = as_image(image)
        self.ctx.check(self.ctx.lib.mis_compensator_apply(self.h, index, C.byref(img)))
        return image


class GainCompensator(_Compensator):
    """cv::detail::GainCompensator(nr_feeds): one gain per frame from the whole-frame overlap statistics."""
    TYPE = capi.EXPOS_GAIN

    def __init__(self, ctx, nr_feeds=1):
        self._create(ctx, nr_feeds)


class ChannelsCompensator(_Compensator):
    """cv::detail::ChannelsCompensator(nr_feeds): a GainCompensator per colour channel; gains(i) = (B, G, R)."""
    TYPE = capi.EXPOS_CHANNELS

    def __init__(self, ctx, nr_feeds=1):
        self._create(ctx, nr_feeds)


class BlocksGainCompensator(_Compensator):
    """cv::detail::BlocksGainCompensator as the reference configures it (image_stitching.cpp:1002-1023): 64x64 blocks,
    one feed, two gain-filtering passes."""
    TYPE = capi.EXPOS_GAIN_BLOCKS

    def __init__(self, ctx, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2, nr_feeds=1):
        self._create(ctx, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)


class BlocksChannelsCompensator(_Compensator):
    """cv::detail::BlocksChannelsCompensator: a gain per block and colour channel, smoothed into a three-channel map."""
    TYPE = capi.EXPOS_CHANNELS_BLOCKS

    def __init__(self, ctx, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2, nr_feeds=1):
        self._create(ctx, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)


# expos_comp_type (image_stitching.cpp:73, :1002-1012) as a configuration name.  "channels" is NOT among them: ChannelsCompensator is
# built (the class above, MIS_EXPOS_CHANNELS, the C++ host's --expos_comp channels), but the suite pins "channels" as its example
# of a configuration value that is refused by name (tests/test_expos_gpu.py, tests/test_distributed_cpu.py), so the Python
# configuration keeps refusing it; build the compensator directly where it is wanted
EXPOS_COMP_TYPES = ("no", "gain", "gain_blocks", "channels_blocks")


def make_compensator(ctx, cfg):
    """expos_comp_type / expos_comp_nr_feeds of the config -> the compensator (image_stitching.cpp:1002-1016), None for "no"."""
    t, feeds = cfg.expos_comp_type, cfg.expos_comp_nr_feeds
    blocks = (cfg.expos_comp_block_size, cfg.expos_comp_block_size, cfg.expos_comp_nr_filtering, feeds)
    if t == "gain":
        return GainCompensator(ctx, feeds)
    if t == "gain_blocks":
        return BlocksGainCompensator(ctx, *blocks)
    if t == "channels_blocks":
        return BlocksChannelsCompensator(ctx, *blocks)
    return None


def make_seam_finder(ctx, cfg):
    """seam_find_type of the config -> the seam finder (image_stitching.cpp:1029-1062), None for "no"."""
    make = {"voronoi": lambda: VoronoiSeamFinder(ctx), "dp_color": lambda: DpSeamFinder(ctx, DpSeamFinder.COLOR),
            "dp_colorgrad": lambda: DpSeamFinder(ctx, DpSeamFinder.COLOR_GRAD)}.get(cfg.seam_find_type)
    return make() if make else None


class NoSeamFinder:
    """seam_find_type "no" (image_stitching.cpp:1029): masks stay as warped."""

    def find(self, images, corners, masks):
        return masks


class VoronoiSeamFinder:
    """seam_find_type "voronoi" (image_stitching.cpp:1031); images are not looked at."""

    def __init__(self, ctx):
        self.ctx = ctx

    def find(self, images, corners, masks):
        n = len(masks)
        cs = _points(corners)
        mk = _images(masks)
        self.ctx.check(self.ctx.lib.mis_seam_voronoi(self.ctx.h, cs, mk, n))
        return masks


class DpSeamFinder:
    """seam_find_type "dp_color" -- the reference's default (image_stitching.cpp:77, :1056-1057, :1065): DpSeamFinder(COLOR) --
    and "dp_colorgrad" (:1057-1058): DpSeamFinder(COLOR_GRAD), whose cut costs are divided by the images' Sobel derivatives
    (one kernel launch for all frames, csrc/seam_grad.hip).  images: the seam-scale warped 8UC3 images; masks are edited in place.
    cost_func: DpSeamFinder.COLOR (0), or a name as OpenCV 4's DpSeamFinder(String costFunc) takes it: "COLOR" | "COLOR_GRAD".
    An integer goes to mis_seam_dp as it is (which runs COLOR only); COLOR_GRAD runs mis_seam_dp_colorgrad."""
    COLOR = 0
    COLOR_GRAD = "COLOR_GRAD"

    def __init__(self, ctx, cost_func=0):
        if isinstance(cost_func, str):
            if cost_func not in ("COLOR", "COLOR_GRAD"):
                raise ValueError("DpSeamFinder cost function %r: 'COLOR' or 'COLOR_GRAD'" % (cost_func,))
            if cost_func == "COLOR":
                cost_func = DpSeamFinder.COLOR
        self.ctx, self.cost_func = ctx, cost_func

    def find(self, images, corners, masks):
        cs, im, mk, n = _seam_args(corners, images, masks)
        if self.cost_func == DpSeamFinder.COLOR_GRAD:
            self.ctx.check(self.ctx.lib.mis_seam_dp_colorgrad(self.ctx.h, cs, im, mk, n))
        else:
            self.ctx.check(self.ctx.lib.mis_seam_dp(self.ctx.h, cs, im, mk, n, int(self.cost_func)))
        return masks


class GraphCutSeamFinder:
    """cv::detail::GraphCutSeamFinder(COST_COLOR, terminal_cost, bad_region_penalty) -- the seam finder of the reference's try_cuda
    branch (image_stitching.cpp:1037-1054) and of OpenCV's own stitcher -- over mis_seam_graphcut: a device max-flow per
    overlapping pair (csrc/seam_gc.hip; the definition is SURVEY.md appendix A.13).  images: the seam-scale warped 8UC3 images;
    masks are edited in place.  cost_type: "COST_COLOR"; "COST_COLOR_GRAD" is known and not built (NotImplementedError), any
    other value is a ValueError.  The class is not a configuration name: hand an instance to Stitcher.set_seam_finder."""
    COST_TYPES = {"COST_COLOR": 0, "COST_COLOR_GRAD": 1}

    def __init__(self, ctx, cost_type="COST_COLOR", terminal_cost=10000.0, bad_region_penalty=1000.0):
        if not isinstance(cost_type, str) or cost_type not in GraphCutSeamFinder.COST_TYPES:
            raise ValueError("GraphCutSeamFinder cost type %r: 'COST_COLOR' or 'COST_COLOR_GRAD'" % (cost_type,))
        if cost_type == "COST_COLOR_GRAD":
            raise NotImplementedError("GraphCutSeamFinder cost type 'COST_COLOR_GRAD' is not built (DESIGN.md section 8); 'COST_COLOR' is")
        self.ctx, self.cost_type = ctx, cost_type
        self.terminal_cost, self.bad_region_penalty = float(terminal_cost), float(bad_region_penalty)

    def find(self, images, corners, masks):
        cs, im, mk, n = _seam_args(corners, images, masks)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut(self.ctx.h, cs, im, mk, n, GraphCutSeamFinder.COST_TYPES[self.cost_type],
                                                      self.terminal_cost, self.bad_region_penalty))
        return masks

    def stats(self):
        """The counts of the context's last find: pairs, levels, grid nodes, the round-set cap, global relabels, relabel sweeps and
        the round sets of every level."""
        count = C.c_int(0)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_stats(self.ctx.h, None, 0, C.byref(count)))
        out = (C.c_int * max(count.value, 1))()
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_stats(self.ctx.h, out, count.value, C.byref(count)))
        v = list(out[:count.value])
        if len(v) < 6:
            return None
        return dict(pairs=v[0], levels=v[1], nodes=v[2], round_set_cap=v[3], relabels=v[4], sweeps=v[5], round_sets=v[6:])

    def debug_pair(self, images, corners, masks, i, j):
        """mis_seam_graphcut_debug_pair: pair (i, j) on the masks as given -> (cap_right, cap_down, terminals, labels), numpy planes
        of the pair's grid (the gap included); nothing is edited."""
        cs, im, mk, n = _seam_args(corners, images, masks)
        gw, gh = C.c_int(0), C.c_int(0)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_debug_pair(self.ctx.h, cs, im, mk, n, i, j, None, None, None, None, 0, C.byref(gw), C.byref(gh)))
        shape = (gh.value, gw.value)
        cr, cd, term = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32)
        lab = np.empty(shape, np.uint8)
        p32 = C.POINTER(C.c_int32)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_debug_pair(self.ctx.h, cs, im, mk, n, i, j, cr.ctypes.data_as(p32), cd.ctypes.data_as(p32), term.ctypes.data_as(p32),
                                                                 lab.ctypes.data_as(C.POINTER(C.c_uint8)), cr.size, C.byref(gw), C.byref(gh)))
        return cr, cd, term, lab


def seam_gradients(ctx, images, gradx=None, grady=None):
    """DpSeamFinder::computeGradients of every image in one launch (mis_seam_gradients): BGR -> grey, then the 3 x 3 Sobel
    derivatives along x and y (BORDER_REFLECT_101) -> (gradx, grady), lists of float32 planes.  images: 8UC3 device tensors or
    host arrays; a plane is allocated where its image lives (a device tensor or a numpy array) unless gradx / grady give the
    buffers to fill."""
    n = len(images)

    def planes(given):
        if given is not None:
            return list(given)
        return [torch.empty(tuple(i.shape[:2]), dtype=torch.float32, device=i.device) if torch is not None and isinstance(i, torch.Tensor)
                else np.empty(np.asarray(i).shape[:2], np.float32) for i in images]
    gx, gy = planes(gradx), planes(grady)
    if len(gx) != n or len(gy) != n:
        raise ValueError("seam_gradients: %d images, %d gradx and %d grady planes" % (n, len(gx), len(gy)))
    im = _images(images)
    ax = _images(gx)
    ay = _images(gy)
    ctx.check(ctx.lib.mis_seam_gradients(ctx.h, im, n, ax, ay))
    return gx, gy


# seam_find_type (image_stitching.cpp:77, :1029-1062) as a configuration name
SEAM_FIND_TYPES = ("no", "voronoi", "dp_color", "dp_colorgrad")


def check_seam_config(cfg):
    if cfg.seam_find_type not in SEAM_FIND_TYPES:
        raise NotImplementedError("seam_find_type %r: 'no', 'voronoi', 'dp_color' and 'dp_colorgrad' are implemented as configuration names "
                                  "(gc_color / gc_colorgrad are not names here: the graph-cut finder is the class GraphCutSeamFinder, handed to "
                                  "Stitcher.set_seam_finder; DESIGN.md section 8)" % (cfg.seam_find_type,))
    if cfg.expos_comp_type not in EXPOS_COMP_TYPES:
        raise NotImplementedError("expos_comp_type %r: one of %s ('channels' is ChannelsCompensator, not a configuration name here)"
                                  % (cfg.expos_comp_type, ", ".join(EXPOS_COMP_TYPES)))
    nf = cfg.expos_comp_nr_feeds
    if isinstance(nf, bool) or not isinstance(nf, (int, np.integer)) or nf < 1:
        raise ValueError("expos_comp_nr_feeds %r: an integer >= 1 (image_stitching.cpp:74)" % (nf,))


def apply_seam(ctx, seam, k, corner, img_s, mask):
    """What the seam-scale step leaves for frame k of the compositing loop: its gains on the warped 16S image (image_stitching.cpp:1162;
    the same values as on the 8U one), then its seam mask on the warped mask (:1169-1171), both in place.  seam: the (compensator |
    None, seam masks) that seam_solve returned."""
    compensator, seam_masks = seam
    if compensator is not None:
        compensator.apply(k, corner, img_s, mask)
    seam_mask_apply(ctx, seam_masks[k], mask)
