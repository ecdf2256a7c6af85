"""What every stage shares: the error type, the context, image marshalling and the owner of a library handle."""
import ctypes as C
import functools

import numpy as np

from . import _capi as capi

try:  # torch is plumbing: device memory + streams
    import torch
except Exception:  # pragma: no cover
    torch = None


class MisError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libmistitch error %d: %s" % (code, text))
        self.code = code


def check_rc(rc, text):
    """The return code of a library call that takes no context (one that does: Context.check) -> MisError(rc, text) unless MIS_OK."""
    if rc != capi.MIS_OK:
        raise MisError(rc, text)


_TORCH_DT = {}
if torch is not None:
    _TORCH_DT = {torch.uint8: capi.U8, torch.int16: capi.S16, torch.float32: capi.F32}
_NP_DT = {np.dtype(np.uint8): capi.U8, np.dtype(np.int16): capi.S16, np.dtype(np.float32): capi.F32}


def _mat9(m):
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(9))
    return a, a.ctypes.data_as(C.c_void_p)


def as_image(a):
    """torch CUDA tensor / numpy array (H,W) or (H,W,C) -> MisImage describing it in place."""
    img = capi.MisImage()
    if torch is not None and isinstance(a, torch.Tensor):
        if a.dim() == 2:
            h, w = a.shape
            c = 1
            assert a.stride(1) == 1, "rows must be dense"
        else:
            h, w, c = a.shape
            assert a.stride(2) == 1 and a.stride(1) == c, "pixels must be dense within a row"
        img.data = a.data_ptr()
        img.stride = a.stride(0) * a.element_size()
        img.dtype = _TORCH_DT[a.dtype]
        img.mem = capi.MEM_DEVICE if a.is_cuda else capi.MEM_HOST
    else:
        a = np.asarray(a)
        if a.ndim == 2:
            h, w = a.shape
            c = 1
            assert a.strides[1] == a.itemsize
        else:
            h, w, c = a.shape
            assert a.strides[2] == a.itemsize and a.strides[1] == c * a.itemsize
        img.data = a.ctypes.data
        img.stride = a.strides[0]
        img.dtype = _NP_DT[a.dtype]
        img.mem = capi.MEM_HOST
    img.width, img.height, img.channels = w, h, c
    return img


def _c_array(ctype, values):
    """values as a C array of ctype; at least one element long, so that n = 0 still hands the library a valid pointer."""
    values = list(values)
    return (ctype * max(len(values), 1))(*values)


def _points(pts):
    return _c_array(capi.MisPoint, (capi.MisPoint(int(p[0]), int(p[1])) for p in pts))


def _images(arrays):
    """The MisImage array of tensors / arrays, which stay the caller's to keep alive for the call."""
    return _c_array(capi.MisImage, (as_image(a) for a in arrays))


def _empty_image(ctx, h, w, c, tdtype):
    """Device image with 256-byte aligned row pitch, returned as a (possibly strided) tensor view."""
    es = torch.empty((), dtype=tdtype).element_size()
    row = w * c * es
    pitch = (row + 255) // 256 * 256
    buf = torch.empty((h, pitch // es), dtype=tdtype, device=ctx.device)
    # as_strided, not view: a view of a single row reports a dense row stride (w * c), which the library refuses for the
    # fused warp's 16SC3 output when w is odd (rows must be 4-byte aligned)
    return buf.as_strided((h, w, c), (pitch // es, c, 1)) if c > 1 else buf[:, : w * c]


@functools.lru_cache(None)
def _hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _memcpy_dtoh(dst_np, dev_ptr, nbytes):
    rc = _hip_runtime().hipMemcpy(dst_np.ctypes.data_as(C.c_void_p), C.c_void_p(dev_ptr), nbytes, 2)
    if rc:
        raise RuntimeError("hipMemcpy D2H failed: %d" % rc)


class Context:
    """One HIP device + one stream (include/mistitch.h: MisContext)."""

    def __init__(self, device=0, stream=None):
        self.lib = capi.load()
        if torch is None:
            raise ImportError("torch is required for device memory management")
        self.device = torch.device("cuda", device)
        if stream is None:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream().cuda_stream
        self.stream = stream
        h = C.c_void_p()
        check_rc(self.lib.mis_context_create(device, C.c_void_p(stream), C.byref(h)),
                 "mis_context_create failed (no HIP device? there is no CPU fallback)")
        self.h = h

    def check(self, rc):
        if rc != capi.MIS_OK:
            raise MisError(rc, self.lib.mis_last_error(self.h).decode())

    def synchronize(self):
        self.check(self.lib.mis_context_synchronize(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mis_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Handle:
    """Owner of one library object created against a context: self.h, freed by the library function the subclass names."""
    DESTROY = None      # "mis_..._destroy"
    h = None

    def close(self):
        h, self.h = self.h, None
        if h and self.ctx.h:   # a destroyed context already released the device (the C object points into it)
            getattr(self.ctx.lib, self.DESTROY)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
