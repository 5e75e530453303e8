"""ctypes binding of include/vio_reject.h (csrc/libvio_reject_hip.so): rejectWithF and undistortedPoints for many streams on the GPU,
the camera-model half of FeatureTracker::readImage (feature_tracker.cpp:169-202 and :258-306).

    rh = vio.load_reject().create()                                  # (device 0, its own stream)
    rh.set_camera(fx=461.6, fy=460.3, cx=363.0, cy=248.1, k1=-0.2917, k2=0.08228, p1=5.333e-05, p2=-1.578e-04, width=752, height=480)
    rh.set_config(seed=0, ransac_hypotheses=128, f_threshold=1.0, focal_length=460.0)
    keep = rh.reject(cur_pts, forw_pts, pair)                        # one pair: a boolean array, True for the pairs to keep
    outs = rh.reject_batch([dict(cur_pts=a, forw_pts=b, pair=k), ...])      # dicts: status, hyp, n_inliers, F (3, 3), mask
    un, vel = rh.undistort(pts, ids, prev_ids, prev_un_pts, dt)      # (n, 2) float32 each
    outs = rh.undistort_batch([dict(pts=, ids=, prev_ids=, prev_un_pts=, dt=), ...])   # dicts: status, un_pts, velocity
    xy = rh.lift(pts)                                                # (n, 2) float64: the bare lift

Points are (n, 2) float32 pixels (x, y); ids are int64 with -1 for a point that has none yet.  A pair or an item with a point that is
not finite gets status NOT_FINITE and does not raise.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError

MAX_POINTS, MAX_ITEMS, MAX_HYPOTHESES, DEFAULT_HYPOTHESES = 4096, 4096, 4096, 128
DEFAULT_F_THRESHOLD, DEFAULT_FOCAL_LENGTH = 1.0, 460.0
LIFT_EVALUATIONS, MIN_POINTS = 8, 8
ROUND, THREADS, ID_CHUNK = 64, 256, 1024
MODEL_PINHOLE = 0
OK, NOT_FINITE, FAIL_NO_MODEL = 0, -3, 1


class VioRejectCamera(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")] + \
               [("width", C.c_int32), ("height", C.c_int32), ("model", C.c_int32), ("reserved", C.c_int32)]


class VioRejectConfig(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("ransac_hypotheses", C.c_int32), ("f_threshold", C.c_double), ("focal_length", C.c_double)]


class VioRejectItem(C.Structure):
    _fields_ = [("n", C.c_int32), ("pair", C.c_uint32), ("cur_pts", C.c_void_p), ("forw_pts", C.c_void_p)]


class VioRejectResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("hyp", C.c_int32), ("n_inliers", C.c_int32), ("reserved", C.c_int32), ("F", C.c_double * 9)]


class VioRejectUndistortItem(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("pts", C.c_void_p), ("ids", C.c_void_p), ("prev_ids", C.c_void_p),
                ("prev_un_pts", C.c_void_p), ("dt", C.c_double), ("un_pts", C.c_void_p), ("velocity", C.c_void_p)]


class RejectLib:
    """libvio_reject_hip.so: vio_reject_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_camera", "set_config", "batch", "undistort_batch", "lift", "timing"]

    def __init__(self, path):
        from .capi import open_lib
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_reject_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_camera"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["undistort_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["lift"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_reject handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return RejectHandle(self, device, stream)


def _pts(a):
    return np.zeros((0, 2), dtype=np.float32) if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 2)


def _ids(a):
    return np.zeros(0, dtype=np.int64) if a is None else np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


class RejectHandle(CompanionHandle):
    PREFIX = "vio_reject_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_reject_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_camera(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, width=752, height=480, model=MODEL_PINHOLE):
        cam = VioRejectCamera(float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(p1), float(p2), int(width), int(height),
                              int(model), 0)
        self._ck(self.lib.fn["set_camera"](self.h, C.byref(cam)), "set_camera")

    def set_config(self, seed=0, ransac_hypotheses=DEFAULT_HYPOTHESES, f_threshold=DEFAULT_F_THRESHOLD, focal_length=DEFAULT_FOCAL_LENGTH):
        cfg = VioRejectConfig(int(seed) & 0xFFFFFFFF, int(ransac_hypotheses), float(f_threshold), float(focal_length))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def reject_batch(self, items):
        """rejectWithF of every pair: a list of dicts status, hyp, n_inliers, F (3, 3), mask (n,) bool."""
        B = len(items)
        arr = (VioRejectItem * max(B, 1))()
        keep = []
        for i, it in enumerate(items):
            a, b = _pts(it["cur_pts"]), _pts(it["forw_pts"])
            if len(a) != len(b):
                raise ValueError("item %d: cur_pts and forw_pts must have one length" % i)
            keep += [a, b]
            arr[i] = VioRejectItem(len(a), int(it.get("pair", 0)) & 0xFFFFFFFF, a.ctypes.data, b.ctypes.data)
        total = sum(int(arr[i].n) for i in range(B))
        mask = np.zeros(max(total, 1), dtype=np.uint8)
        res = (VioRejectResult * max(B, 1))()
        st = self.lib.fn["batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res), mask.ctypes.data)
        self._ck(st, "batch", allow_not_finite=True)
        out, o = [], 0
        for i in range(B):
            r, n = res[i], int(arr[i].n)
            out.append(dict(status=int(r.status), hyp=int(r.hyp), n_inliers=int(r.n_inliers), F=np.array(r.F, dtype=np.float64).reshape(3, 3),
                            mask=mask[o:o + n].astype(bool)))
            o += n
        return out

    def reject(self, cur_pts, forw_pts, pair=0):
        """The pairs to keep: (n,) bool (FeatureTracker's rejecter interface)."""
        return self.reject_batch([dict(cur_pts=cur_pts, forw_pts=forw_pts, pair=pair)])[0]["mask"]

    def undistort_batch(self, items):
        """undistortedPoints of every item: a list of dicts status, un_pts (n, 2) float32, velocity (n, 2) float32."""
        B = len(items)
        arr = (VioRejectUndistortItem * max(B, 1))()
        keep, outs = [], []
        for i, it in enumerate(items):
            p, ids = _pts(it["pts"]), _ids(it.get("ids"))
            pi, pu = _ids(it.get("prev_ids")), _pts(it.get("prev_un_pts"))
            if len(ids) != len(p) or len(pi) != len(pu):
                raise ValueError("item %d: ids needs one entry per point, prev_ids one per previous point" % i)
            un = np.full((max(len(p), 1), 2), np.nan, dtype=np.float32)
            vel = np.full((max(len(p), 1), 2), np.nan, dtype=np.float32)
            keep += [p, ids, pi, pu]
            outs.append((un, vel, len(p)))
            dt = it.get("dt")
            arr[i] = VioRejectUndistortItem(len(p), len(pi), p.ctypes.data, ids.ctypes.data, pi.ctypes.data, pu.ctypes.data,
                                            float(0.0 if dt is None else dt), un.ctypes.data, vel.ctypes.data)
        status = (C.c_int32 * max(B, 1))()
        st = self.lib.fn["undistort_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(status))
        self._ck(st, "undistort_batch", allow_not_finite=True)
        return [dict(status=int(status[i]), un_pts=un[:n].copy(), velocity=vel[:n].copy()) for i, (un, vel, n) in enumerate(outs)]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        """(un_pts, velocity) of one point set (FeatureTracker's rejecter interface)."""
        if ids is None:
            ids = np.full(len(_pts(pts)), -1, dtype=np.int64)
        o = self.undistort_batch([dict(pts=pts, ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un_pts, dt=dt)])[0]
        return o["un_pts"], o["velocity"]

    def lift(self, pts):
        """The bare lift: (n, 2) float64."""
        p = _pts(pts)
        out = np.zeros((max(len(p), 1), 2), dtype=np.float64)
        self._ck(self.lib.fn["lift"](self.h, C.c_int32(len(p)), p.ctypes.data, out.ctypes.data), "lift")
        return out[:len(p)]

    def timing(self):
        """ms of the last call that launched: host packing + upload, the kernel, the whole call."""
        t = (C.c_double * 3)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"upload_ms": t[0], "kernel_ms": t[1], "total_ms": t[2]}
