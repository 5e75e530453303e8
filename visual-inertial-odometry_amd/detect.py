"""ctypes binding of include/vio_detect.h (csrc/libvio_detect_hip.so): Shi-Tomasi corner detection with setMask for many images on the
GPU, the steps of FeatureTracker::readImage that replace lost keypoints (feature_tracker.cpp:36-69 and :149).

    dh = vio.load_detect().create()                                  # (device 0, its own stream)
    dh.set_config(quality=0.01, min_distance=30)
    out = dh.detect(img, tracked=pts, track_cnt=cnt, mask=None, max_total=150)      # one image: a dict
    outs = dh.detect_batch([dict(img=a, tracked=p, track_cnt=c, mask=m, max_total=150), ...])
    R = dh.response(img)                                             # the float64 response map of one image

An item is a dict: img (height, width) uint8 (rows may be strided), tracked (n, 2) float32 as (x, y) or None, track_cnt (n,) int32,
mask like img or None, max_total.  A result is a dict: status, keep_order (n_kept,) int32 (the indices of the tracked points setMask
keeps, in output order), new_pts (n_new, 2) float32, n_kept, n_new, n_candidates, max_response.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib
from .flow import _image

MAX_DIM, MAX_POINTS = 16384, 4096
BLOCK, APERTURE = 3, 3
DEFAULT_QUALITY, DEFAULT_MIN_DISTANCE, DEFAULT_MAX_TOTAL = 0.01, 30, 150
TILE_X, TILE_Y = 32, 8
OK, NOT_FINITE = 0, -3


class VioDetectConfig(C.Structure):
    _fields_ = [("quality", C.c_double), ("min_distance", C.c_int32), ("reserved", C.c_int32)]


class VioDetectItem(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("n_tracked", C.c_int32), ("max_total", C.c_int32),
                ("reserved", C.c_int32), ("img", C.c_void_p), ("mask", C.c_void_p), ("tracked", C.c_void_p), ("track_cnt", C.c_void_p),
                ("keep_order", C.c_void_p), ("new_pts", C.c_void_p)]


class VioDetectResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_kept", C.c_int32), ("n_new", C.c_int32), ("n_candidates", C.c_int32),
                ("max_response", C.c_double)]


class DetectLib:
    """libvio_detect_hip.so: vio_detect_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "batch", "response", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_detect_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["response"].argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_detect handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return DetectHandle(self, device, stream)


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items)."""

    def __init__(self, items):
        self.keep = []
        self.items = (VioDetectItem * max(1, len(items)))()
        self.keep_order, self.new_pts = [], []
        for i, it in enumerate(items):
            a = _image(it["img"])
            m = None if it.get("mask") is None else _image(it["mask"])
            if m is not None and m.shape != a.shape:
                raise ValueError("item %d: img and mask must have one shape" % i)
            if m is not None and m.strides[0] != a.strides[0]:
                a, m = np.ascontiguousarray(a), np.ascontiguousarray(m)
            trk = it.get("tracked")
            pts = np.zeros((0, 2), dtype=np.float32) if trk is None else np.ascontiguousarray(trk, dtype=np.float32).reshape(-1, 2)
            cnt = it.get("track_cnt")
            cnt = np.ones(len(pts), dtype=np.int32) if cnt is None else np.ascontiguousarray(cnt, dtype=np.int32).reshape(-1)
            if len(cnt) != len(pts):
                raise ValueError("item %d: track_cnt needs one entry per tracked point" % i)
            max_total = int(it.get("max_total", DEFAULT_MAX_TOTAL))
            ko = np.full(max(len(pts), 1), -1, dtype=np.int32)
            npt = np.full((max(max_total, 1), 2), np.nan, dtype=np.float32)
            self.keep += [a, m, pts, cnt]
            self.keep_order.append(ko)
            self.new_pts.append(npt)
            self.items[i] = VioDetectItem(a.shape[1], a.shape[0], a.strides[0], len(pts), max_total, 0, a.ctypes.data,
                                          None if m is None else m.ctypes.data, pts.ctypes.data, cnt.ctypes.data, ko.ctypes.data,
                                          npt.ctypes.data)


class DetectHandle(CompanionHandle):
    PREFIX = "vio_detect_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_detect_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, quality=DEFAULT_QUALITY, min_distance=DEFAULT_MIN_DISTANCE):
        cfg = VioDetectConfig(float(quality), int(min_distance), 0)
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def detect_batch(self, items):
        """setMask and the new corners of every item: a list of dicts (module docstring).  An item with a non-finite tracked point
        gets status NOT_FINITE and nothing else; it does not raise."""
        B = len(items)
        pk = _Packed(items)
        res = (VioDetectResult * max(B, 1))()
        st = self.lib.fn["batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(res))
        self._ck(st, "batch", allow_not_finite=True)
        out = []
        for i in range(B):
            r = res[i]
            out.append(dict(status=int(r.status), n_kept=int(r.n_kept), n_new=int(r.n_new), n_candidates=int(r.n_candidates),
                            max_response=float(r.max_response), keep_order=pk.keep_order[i][:r.n_kept].copy(),
                            new_pts=pk.new_pts[i][:r.n_new].copy()))
        return out

    def detect(self, img, tracked=None, track_cnt=None, mask=None, max_total=DEFAULT_MAX_TOTAL):
        return self.detect_batch([dict(img=img, tracked=tracked, track_cnt=track_cnt, mask=mask, max_total=max_total)])[0]

    def response(self, img):
        """The response map of one image: (height, width) float64."""
        a = _image(img)
        h, w = a.shape
        out = np.zeros((max(h, 1), max(w, 1)), dtype=np.float64)
        self._ck(self.lib.fn["response"](self.h, a.ctypes.data, C.c_int32(w), C.c_int32(h), C.c_int32(a.strides[0]), out.ctypes.data), "response")
        return out

    def timing(self):
        """ms of the last detect_batch that launched: host packing + upload, the four kernels, the whole call."""
        t = (C.c_double * 6)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"upload_ms": t[0], "setmask_ms": t[1], "response_ms": t[2], "candidates_ms": t[3], "select_ms": t[4], "total_ms": t[5]}
