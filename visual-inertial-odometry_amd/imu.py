"""ctypes binding of include/vio_imu.h (csrc/libvio_imu_hip.so): batched IMU pre-integration and bias re-propagation on the GPU.

    h = load_imu().create()                      # a handle on device 0, on a stream of its own
    h.load(intervals, noise)                     # the dicts stream.cut_imu_intervals returns (acc0, gyr0, dt, acc, gyr): uploaded once
    pres = h.propagate(ba, bg)                   # IntegrationBase over every interval at biases ba, bg ((3,) or (n, 3)): n VioPreint
    pres = h.propagate(ba, bg, which=[3, 7])     # ... re-propagation of a subset: the records of intervals 3 and 7

The records are what VioContext.set_imu_all takes.
"""
import ctypes as C

import numpy as np

from . import synth
from .capi import CompanionHandle, VioError, VioPreint, open_lib


class VioImuNoise(C.Structure):
    _fields_ = [("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double)]


class ImuLib:
    """libvio_imu_hip.so: vio_imu_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "load", "propagate", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_imu_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["load"].argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        self.fn["propagate"].argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_imu handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return ImuHandle(self, device, stream)


def pack_intervals(intervals):
    """The CSR arrays of vio_imu_load: offset (n + 1,) int64, first (n, 6), dt (S,), acc (S, 3), gyr (S, 3)."""
    n = len(intervals)
    counts = [len(iv["dt"]) for iv in intervals]
    offset = np.zeros(n + 1, dtype=np.int64)
    offset[1:] = np.cumsum(counts, dtype=np.int64)
    first = np.zeros((n, 6))
    for i, iv in enumerate(intervals):
        first[i, 0:3] = np.asarray(iv["acc0"], dtype=np.float64).reshape(3)
        first[i, 3:6] = np.asarray(iv["gyr0"], dtype=np.float64).reshape(3)
    S = int(offset[-1])
    cat = lambda key, w: (np.ascontiguousarray(np.concatenate([np.asarray(iv[key], dtype=np.float64).reshape(-1, w)
                                                              for iv in intervals if len(iv["dt"])]).reshape(S, w))
                          if S else np.zeros((0, w)))
    return offset, first, cat("dt", 1).reshape(S), cat("acc", 3), cat("gyr", 3)


def record_dict(p):
    """A VioPreint as the dict synth.preintegrate returns (what StreamDriver and synth.Window carry)."""
    v = np.frombuffer(p, dtype=np.float64).copy()
    return {"sum_dt": float(v[0]), "delta_p": v[1:4], "delta_q": v[4:8], "delta_v": v[8:11], "linearized_ba": v[11:14],
            "linearized_bg": v[14:17], "jacobian": v[17:242].reshape(15, 15), "covariance": v[242:467].reshape(15, 15)}


class ImuHandle(CompanionHandle):
    PREFIX = "vio_imu_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        self.n = None
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_imu_create")

    def load(self, intervals, noise=None):
        """Upload the raw samples of `intervals` (dicts with acc0, gyr0, dt, acc, gyr).  noise: dict acc_n, gyr_n, acc_w, gyr_w
        (default: synth's, as synth.preintegrate)."""
        nz = dict(acc_n=synth.ACC_N, gyr_n=synth.GYR_N, acc_w=synth.ACC_W, gyr_w=synth.GYR_W)
        nz.update(noise or {})
        offset, first, dt, acc, gyr = pack_intervals(intervals)
        n = len(intervals)
        cn = VioImuNoise(float(nz["acc_n"]), float(nz["gyr_n"]), float(nz["acc_w"]), float(nz["gyr_w"]))
        ptr = lambda a: a.ctypes.data if a.size else None
        self._ck(self.lib.fn["load"](self.h, C.c_int32(n), offset.ctypes.data, ptr(first), ptr(dt), ptr(acc), ptr(gyr),
                                     C.byref(cn)), "load")
        self.n = n

    def propagate(self, ba, bg, which=None, out=None):
        """IntegrationBase at biases ba / bg ((3,): every interval, or (n, 3)) over the intervals listed in `which` (None: all).
        out: optional (VioPreint * n) array the records are written into (only the listed entries are touched).  Returns the records
        of the listed intervals, in `which`'s order.  A non-finite record raises VioError (out holds the records all the same)."""
        if self.n is None:
            raise VioError(-1, "vio_imu_propagate", "(nothing loaded)")
        n = self.n
        ba = np.ascontiguousarray(np.broadcast_to(np.asarray(ba, dtype=np.float64), (n, 3)))
        bg = np.ascontiguousarray(np.broadcast_to(np.asarray(bg, dtype=np.float64), (n, 3)))
        if out is None:
            out = (VioPreint * max(n, 1))()
        elif not (isinstance(out, C.Array) and out._type_ is VioPreint and len(out) >= n):
            raise ValueError("out: a (VioPreint * %d) array" % n)
        if which is not None and len(which) == 0:
            return []
        if which is None:
            idx = list(range(n))
            st = self.lib.fn["propagate"](self.h, C.c_int32(n), None, ba.ctypes.data, bg.ctypes.data, C.addressof(out))
        else:
            w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
            idx = [int(i) for i in w]
            st = self.lib.fn["propagate"](self.h, C.c_int32(w.size), w.ctypes.data if w.size else None, ba.ctypes.data,
                                          bg.ctypes.data, C.addressof(out))
        self._ck(st, "propagate")
        return [out[i] for i in idx]

    def timing(self):
        """ms of the last propagate: host packing + upload, k_imu_propagate, the whole call."""
        t = (C.c_double * 3)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "total_ms": t[2]}
