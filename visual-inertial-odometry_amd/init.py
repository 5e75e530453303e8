"""ctypes binding of include/vio_init.h (csrc/libvio_init_hip.so): visual-inertial alignment of many windows on the GPU.

    ih = vio.load_init().create()                            # (device 0, its own stream)
    bg = ih.gyro_bias_batch(items)                           # solveGyroscopeBias of every window: (B, 3)
    out = ih.align_batch(items, tic, g_norm, bg)             # LinearAlignment + RefineGravity + the state change: one dict per window
    out = ih.initialize_batch(items, intervals, imu, tic, g_norm)    # the whole VisualIMUAlignment: gyro, re-propagation, align

An item is a dict: R (F, 3, 3) = ImageFrame::R, T (F, 3) = ImageFrame::T (up to scale), pre (F-1 records: VioPreint or the dicts
synth.preintegrate returns; pre[k] is interval k -> k+1), is_key (F,) or None (every frame a keyframe).  stream.visual_trajectory makes
R / T from a stream's ground truth, as initialStructure would leave them.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, VioPreint, open_lib
from .imu import record_dict

MAX_FRAMES = 32
X_STRIDE = 3 * MAX_FRAMES + 3
POSE_STRIDE = 7 * MAX_FRAMES
SB_STRIDE = 9 * MAX_FRAMES
OK, NOT_FINITE = 0, -3
FAIL_GRAVITY, FAIL_SCALE, FAIL_REFINED_SCALE = 1, 2, 3
STATUS_NAMES = {OK: "ok", NOT_FINITE: "not finite", FAIL_GRAVITY: "linear stage: | |g| - G | > 1", FAIL_SCALE: "linear stage: s < 0",
                FAIL_REFINED_SCALE: "refined stage: s < 0"}


class VioInitItem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("is_key", C.c_void_p), ("R", C.c_void_p), ("T", C.c_void_p), ("pre", C.c_void_p)]


class VioInitResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_key", C.c_int32), ("s", C.c_double), ("g", C.c_double * 3), ("g_world", C.c_double * 3),
                ("s_linear", C.c_double), ("g_linear", C.c_double * 3), ("rot", C.c_double * 9)]


class InitLib:
    """libvio_init_hip.so: vio_init_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "gyro_bias_batch", "align_batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_init_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["gyro_bias_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["align_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_init handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return InitHandle(self, device, stream)


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items)."""

    def __init__(self, items):
        self.keep = []
        self.items = (VioInitItem * max(1, len(items)))()
        for i, it in enumerate(items):
            R = np.ascontiguousarray(it["R"], dtype=np.float64).reshape(-1, 9)
            T = np.ascontiguousarray(it["T"], dtype=np.float64).reshape(-1, 3)
            F = len(R)
            pre = (VioPreint * max(1, F - 1))()
            for k, p in enumerate(it["pre"][:F - 1]):
                pre[k] = VioPreint.from_dict(p)
            key = it.get("is_key")
            key = None if key is None else np.ascontiguousarray(np.asarray(key, dtype=bool), dtype=np.uint8)
            self.keep += [R, T, pre, key]
            self.items[i] = VioInitItem(F, key.ctypes.data if key is not None else None, R.ctypes.data, T.ctypes.data,
                                        C.addressof(pre))


class InitHandle(CompanionHandle):
    PREFIX = "vio_init_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_init_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def gyro_bias_batch(self, items, bg_in=None, status=False):
        """solveGyroscopeBias of every window: bg_in + delta_bg, (B, 3) (bg_in default zero: Bgs[] at the start).  status=True: also
        the per-window status array (a non-finite window is NaN and VIO_ERR_NOT_FINITE; no exception)."""
        B = len(items)
        bg_in = np.ascontiguousarray(np.broadcast_to(np.zeros(3) if bg_in is None else np.asarray(bg_in, dtype=np.float64), (B, 3)))
        out = np.zeros((max(B, 1), 3))
        sts = np.zeros(max(B, 1), dtype=np.int32)
        pk = _Packed(items)
        st = self.lib.fn["gyro_bias_batch"](self.h, C.c_int32(B), C.addressof(pk.items), bg_in.ctypes.data, out.ctypes.data,
                                            sts.ctypes.data)
        self._ck(st, "gyro_bias_batch", allow_not_finite=status)
        return (out[:B], sts[:B]) if status else out[:B]

    def align_batch(self, items, tic, g_norm, bg):
        """LinearAlignment + RefineGravity + visualInitialAlign's state change for every window: a list of dicts (status, n_key, s,
        g, g_world, s_linear, g_linear, rot (3 x 3), x (3F+3), poses (K x 7), speed_bias (K x 9)).  Non-finite windows do not raise."""
        B = len(items)
        tic = np.ascontiguousarray(tic, dtype=np.float64).reshape(3)
        bg = np.ascontiguousarray(np.broadcast_to(np.asarray(bg, dtype=np.float64), (B, 3)))
        res = (VioInitResult * max(B, 1))()
        x = np.full((max(B, 1), X_STRIDE), np.nan)
        poses = np.full((max(B, 1), POSE_STRIDE), np.nan)
        sb = np.full((max(B, 1), SB_STRIDE), np.nan)
        pk = _Packed(items)
        st = self.lib.fn["align_batch"](self.h, C.c_int32(B), C.addressof(pk.items), tic.ctypes.data, C.c_double(g_norm),
                                        bg.ctypes.data, C.addressof(res), x.ctypes.data, poses.ctypes.data, sb.ctypes.data)
        self._ck(st, "align_batch", allow_not_finite=True)
        out = []
        for i, it in enumerate(items):
            r = res[i]
            F, K = len(np.asarray(it["R"]).reshape(-1, 9)), r.n_key
            out.append(dict(status=int(r.status), n_key=int(K), s=r.s, g=np.array(r.g[:]), g_world=np.array(r.g_world[:]),
                            s_linear=r.s_linear, g_linear=np.array(r.g_linear[:]), rot=np.array(r.rot[:]).reshape(3, 3),
                            x=x[i, :3 * F + 3].copy(), poses=poses[i, :7 * K].reshape(K, 7).copy(),
                            speed_bias=sb[i, :9 * K].reshape(K, 9).copy()))
        return out

    def initialize_batch(self, items, intervals, imu, tic, g_norm, noise=None):
        """The whole VisualIMUAlignment of every window: one gyro launch; one imu.load of every window's raw intervals (intervals[i]:
        the F-1 dicts of window i, as stream.cut_imu_intervals makes them); one propagate at each window's new bias (ba = 0:
        repropagate(Vector3d::Zero(), Bgs[0])); one align launch.  imu: an ImuHandle.  Returns align_batch's dicts, each with `bg`
        and `pre` (the re-propagated records, as dicts) added."""
        B = len(items)
        if B == 0:
            return []
        bg, gst = self.gyro_bias_batch(items, status=True)
        flat, owner = [], []
        for i in range(B):
            flat.extend(intervals[i])
            owner.extend([i] * len(intervals[i]))
        imu.load(flat, noise)
        bgs = np.nan_to_num(bg[np.array(owner)], nan=0.0) if flat else np.zeros((0, 3))
        recs = imu.propagate(np.zeros(3), bgs) if flat else []
        pres, k = [], 0
        for i in range(B):
            n = len(intervals[i])
            pres.append(recs[k:k + n])
            k += n
        items2 = [dict(it, pre=pres[i]) for i, it in enumerate(items)]
        out = self.align_batch(items2, tic, g_norm, np.nan_to_num(bg, nan=0.0))
        for i, o in enumerate(out):
            o["bg"] = bg[i].copy()
            o["pre"] = [record_dict(r) for r in pres[i]]
            if gst[i] != OK:           # the gyro step failed: nothing after it holds (the align ran at bg = 0 for the batch's sake)
                o["status"] = NOT_FINITE
                for k in ("s", "s_linear"):
                    o[k] = np.nan
                for k in ("g", "g_world", "g_linear", "rot", "x", "poses", "speed_bias"):
                    o[k] = np.full_like(o[k], np.nan)
        return out

    def timing(self):
        """ms of the last call: host packing + upload, the kernel (device events), the whole call."""
        t = (C.c_double * 3)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "total_ms": t[2]}
