"""ctypes binding of include/vio_flow.h (csrc/libvio_flow_hip.so): pyramidal Lucas-Kanade tracking of the keypoints of many image pairs
on the GPU, the step of FeatureTracker::readImage that makes the tracks (feature_tracker.cpp:108-125).

    fh = vio.load_flow().create()                                    # (device 0, its own stream)
    fh.set_config(levels=4, half_patch=4, inverse=1)
    out = fh.track(img_prev, img_next, prev_pts)                     # one pair: a dict
    outs = fh.track_batch([dict(img_prev=a, img_next=b, prev_pts=p, guess=None), ...])
    levels = fh.pyramid(img)                                         # the uint8 levels of one image

    fh.set_back(levels=2, max_dist=0.5)                              # the forward-backward check (include/vio_flow_back.h)
    out = fh.track(img_prev, img_next, prev_pts, back=True)          # ... and its rows: back_pts, back_status, back_d2, ...

An item is a dict: img_prev, img_next (height, width) uint8 of one shape (rows may be strided), prev_pts (n, 2) float32 as (x, y),
guess (n, 2) or None.  A result is a dict: next_pts (n, 2) float32, status (n,), iterations (n,), cost (n,).
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib

MAX_LEVELS, MAX_HALF_PATCH, MAX_POINTS, MAX_DIM = 8, 16, 4096, 16384
DEFAULT_LEVELS, DEFAULT_HALF_PATCH, DEFAULT_MAX_ITER, DEFAULT_BORDER = 4, 4, 10, 1
OK, NOT_FINITE = 0, -3
FAIL_LOST, FAIL_BORDER = 1, 2
FAIL_BACK_LOST, FAIL_BACK_FAR, BACK_NOT_RUN = 3, 4, -1               # include/vio_flow_back.h
DEFAULT_BACK_MAX_DIST = 0.5
STATUS_NAMES = {OK: "ok", NOT_FINITE: "not finite", FAIL_LOST: "lost", FAIL_BORDER: "outside the border",
                FAIL_BACK_LOST: "lost on the way back", FAIL_BACK_FAR: "came back too far off"}


class VioFlowConfig(C.Structure):
    _fields_ = [("levels", C.c_int32), ("half_patch", C.c_int32), ("max_iter", C.c_int32), ("inverse", C.c_int32), ("border", C.c_int32),
                ("early_stop", C.c_int32)]


class VioFlowItem(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("n_pts", C.c_int32), ("img_prev", C.c_void_p),
                ("img_next", C.c_void_p), ("prev_pts", C.c_void_p), ("guess", C.c_void_p)]


class VioFlowPtInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("cost", C.c_double)]


class VioFlowBackConfig(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("levels", C.c_int32), ("max_dist", C.c_double)]


class VioFlowBackInfo(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("status", C.c_int32), ("iterations", C.c_int32), ("cost", C.c_double), ("d2", C.c_double)]


PT_INFO_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("cost", np.float64)])
BACK_INFO_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("status", np.int32), ("iterations", np.int32), ("cost", np.float64),
                            ("d2", np.float64)])


def track_results(base, nxt, info, back=None):
    """The dicts of track_batch from the flat arrays a track call filled; base: the items' first rows and the total."""
    total = max(int(base[-1]), 1)
    rec = np.frombuffer(info, dtype=PT_INFO_DTYPE, count=total)
    brec = None if back is None else np.frombuffer(back, dtype=BACK_INFO_DTYPE, count=total)
    out = []
    for i in range(len(base) - 1):
        lo, hi = int(base[i]), int(base[i + 1])
        d = dict(next_pts=nxt[lo:hi].copy(), status=rec["status"][lo:hi].copy(), iterations=rec["iterations"][lo:hi].copy(),
                 cost=rec["cost"][lo:hi].copy())
        if brec is not None:
            d.update(back_pts=np.stack([brec["x"][lo:hi], brec["y"][lo:hi]], axis=1), back_status=brec["status"][lo:hi].copy(),
                     back_iterations=brec["iterations"][lo:hi].copy(), back_cost=brec["cost"][lo:hi].copy(), back_d2=brec["d2"][lo:hi].copy())
        out.append(d)
    return out


class FlowLib:
    """libvio_flow_hip.so: vio_flow_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "track_batch", "pyramid", "timing"]
    BACK_SYMBOLS = ["set_back", "track_back_batch"]                  # include/vio_flow_back.h

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_flow_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["track_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["pyramid"].argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_flow_", self.BACK_SYMBOLS)[1])
        self.fn["set_back"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["track_back_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_flow handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return FlowHandle(self, device, stream)


def _image(a):
    """A uint8 image whose rows are contiguous (the rows themselves may be strided)."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("an image must be a 2-d uint8 array")
    if a.shape[1] > 1 and a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items)."""

    def __init__(self, items):
        self.keep = []
        self.items = (VioFlowItem * max(1, len(items)))()
        self.n = []
        for i, it in enumerate(items):
            a, b = _image(it["img_prev"]), _image(it["img_next"])
            if a.shape != b.shape:
                raise ValueError("item %d: img_prev and img_next must have one shape" % i)
            if a.strides[0] != b.strides[0]:
                a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            pts = np.ascontiguousarray(it["prev_pts"], dtype=np.float32).reshape(-1, 2)
            g = None if it.get("guess") is None else np.ascontiguousarray(it["guess"], dtype=np.float32).reshape(-1, 2)
            if g is not None and len(g) != len(pts):
                raise ValueError("item %d: guess needs one row per keypoint" % i)
            n = int(it.get("n_pts", len(pts)))
            self.keep += [a, b, pts, g]
            self.n.append(max(n, 0))
            self.items[i] = VioFlowItem(a.shape[1], a.shape[0], a.strides[0], n, a.ctypes.data, b.ctypes.data, pts.ctypes.data,
                                        None if g is None else g.ctypes.data)
        self.total = sum(self.n)
        self.base = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)


class FlowHandle(CompanionHandle):
    PREFIX = "vio_flow_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        self.levels = DEFAULT_LEVELS
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_flow_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, levels=DEFAULT_LEVELS, half_patch=DEFAULT_HALF_PATCH, max_iter=DEFAULT_MAX_ITER, inverse=0, border=DEFAULT_BORDER,
                   early_stop=0):
        cfg = VioFlowConfig(int(levels), int(half_patch), int(max_iter), int(inverse), int(border), int(early_stop))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")
        self.levels = int(levels)

    def set_back(self, enabled=True, levels=0, max_dist=DEFAULT_BACK_MAX_DIST):
        """The forward-backward check (include/vio_flow_back.h): every keypoint that tracked is followed back over `levels` levels (0: the
        handle's) and kept only if it ends within max_dist of where it started.  With it on, track and track_batch apply it."""
        cfg = VioFlowBackConfig(1 if enabled else 0, int(levels), float(max_dist))
        self._ck(self.lib.fn["set_back"](self.h, C.byref(cfg)), "set_back")

    def track_batch(self, items, back=False):
        """The keypoints of every pair followed from img_prev into img_next: a list of dicts (next_pts (n, 2) float32: the position the
        reference leaves, tracked or not; status (n,): OK, FAIL_LOST, FAIL_BORDER or NOT_FINITE, and with the check FAIL_BACK_LOST or
        FAIL_BACK_FAR; iterations (n,) and cost (n,) of level 0).  Non-finite keypoints do not raise.  back=True (the check must be
        on: set_back): also back_pts (n, 2) float32, back_status (n,): OK, FAIL_LOST or BACK_NOT_RUN, back_iterations, back_cost and
        back_d2 (n,), the squared distance the verdict compares."""
        B = len(items)
        pk = _Packed(items)
        nxt = np.full((max(pk.total, 1), 2), np.nan, dtype=np.float32)
        info = (VioFlowPtInfo * max(pk.total, 1))()
        binfo = None
        if back:
            binfo = (VioFlowBackInfo * max(pk.total, 1))()
            st = self.lib.fn["track_back_batch"](self.h, C.c_int32(B), C.addressof(pk.items), nxt.ctypes.data, C.addressof(info), C.addressof(binfo))
        else:
            st = self.lib.fn["track_batch"](self.h, C.c_int32(B), C.addressof(pk.items), nxt.ctypes.data, C.addressof(info))
        self._ck(st, "track_back_batch" if back else "track_batch", allow_not_finite=True)
        return track_results(pk.base, nxt, info, binfo)

    def track(self, img_prev, img_next, prev_pts, guess=None, back=False):
        return self.track_batch([dict(img_prev=img_prev, img_next=img_next, prev_pts=prev_pts, guess=guess)], back=back)[0]

    def pyramid(self, img):
        """The configured levels of one image, level 0 first: a list of uint8 arrays."""
        a = _image(img)
        h, w = a.shape
        sizes = [(w, h)]
        for _ in range(self.levels - 1):
            sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
        out = np.zeros(max(1, sum(max(x, 0) * max(y, 0) for x, y in sizes)), dtype=np.uint8)
        self._ck(self.lib.fn["pyramid"](self.h, a.ctypes.data, C.c_int32(w), C.c_int32(h), C.c_int32(a.strides[0]), out.ctypes.data), "pyramid")
        res, off = [], 0
        for x, y in sizes:
            res.append(out[off:off + x * y].reshape(y, x).copy())
            off += x * y
        return res

    def timing(self):
        """ms of the last call that launched: host packing + upload, the pyramid kernels, k_flow_track, the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"upload_ms": t[0], "pyramid_ms": t[1], "track_ms": t[2], "total_ms": t[3]}
