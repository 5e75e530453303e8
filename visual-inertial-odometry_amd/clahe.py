"""ctypes binding of include/vio_clahe.h (csrc/libvio_clahe_hip.so): CLAHE equalisation of many 8-bit images on the GPU, the first step
of FeatureTracker::readImage with EQUALIZE set (feature_tracker.cpp:87-95).

    ch = vio.load_clahe().create()                                   # (device 0, its own stream)
    ch.set_config(clip_limit=3.0, tiles=(8, 8))
    out = ch.apply(img)                                              # one image: uint8 of the same shape
    outs = ch.apply_batch([img_a, img_b, ...])                       # the images may differ in size
    res = ch.apply_batch([img_a, ...], luts=True)                    # dicts: out, luts (tiles_y, tiles_x, 256) uint8, clip, tile_w, tile_h

An image is a (height, width) uint8 array; its rows may be strided.  `out=` takes the arrays the results are written to (of the images'
shapes, rows may be strided too).  A handle is what frontend.FeatureTracker takes as `equalizer`.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib
from .flow import _image

MAX_DIM, MAX_TILES, BINS = 16384, 16, 256
DEFAULT_CLIP_LIMIT, DEFAULT_TILES = 3.0, 8
TILE_X, TILE_Y = 128, 16


class VioClaheConfig(C.Structure):
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32)]


class VioClaheItem(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("src_stride", C.c_int32), ("dst_stride", C.c_int32), ("src", C.c_void_p),
                ("dst", C.c_void_p), ("luts", C.c_void_p)]


class VioClaheResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("clip", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32)]


class ClaheLib:
    """libvio_clahe_hip.so: vio_clahe_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "apply_batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_clahe_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["apply_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_clahe handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return ClaheHandle(self, device, stream)


class ClaheHandle(CompanionHandle):
    PREFIX = "vio_clahe_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        self.tiles = (DEFAULT_TILES, DEFAULT_TILES)
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_clahe_create")

    def set_config(self, clip_limit=DEFAULT_CLIP_LIMIT, tiles=(DEFAULT_TILES, DEFAULT_TILES)):
        """tiles: (tiles_x, tiles_y)."""
        cfg = VioClaheConfig(float(clip_limit), int(tiles[0]), int(tiles[1]))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")
        self.tiles = (int(tiles[0]), int(tiles[1]))

    def apply_batch(self, images, luts=False, out=None):
        """The equalised images: a list of uint8 arrays, or with luts=True a list of dicts (module docstring)."""
        B = len(images)
        if out is not None and len(out) != B:
            raise ValueError("out needs one array per image")
        items = (VioClaheItem * max(B, 1))()
        res = (VioClaheResult * max(B, 1))()
        src, dst, tab = [], [], []
        for i, im in enumerate(images):
            a = _image(im)
            o = np.empty(a.shape, dtype=np.uint8) if out is None else out[i]
            if not isinstance(o, np.ndarray) or o.dtype != np.uint8 or o.shape != a.shape or (o.shape[1] > 1 and o.strides[1] != 1) or \
                    o.strides[0] < o.shape[1] or not o.flags.writeable:
                raise ValueError("out[%d] must be a writeable uint8 array of the image's shape with contiguous rows" % i)
            t = np.zeros((self.tiles[1], self.tiles[0], BINS), dtype=np.uint8) if luts else None
            src.append(a); dst.append(o); tab.append(t)
            items[i] = VioClaheItem(a.shape[1], a.shape[0], a.strides[0], o.strides[0], a.ctypes.data, o.ctypes.data,
                                    None if t is None else t.ctypes.data)
        self._ck(self.lib.fn["apply_batch"](self.h, C.c_int32(B), C.addressof(items), C.addressof(res)), "apply_batch")
        if not luts:
            return dst
        return [dict(status=int(res[i].status), out=dst[i], luts=tab[i], clip=int(res[i].clip), tile_w=int(res[i].tile_w),
                     tile_h=int(res[i].tile_h)) for i in range(B)]

    def apply(self, img):
        return self.apply_batch([img])[0]

    def timing(self):
        """ms of the last apply_batch that launched: host packing + upload, the two kernels, the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"upload_ms": t[0], "lut_ms": t[1], "apply_ms": t[2], "total_ms": t[3]}
