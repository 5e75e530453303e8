"""ctypes binding of include/vio_exrot.h (csrc/libvio_exrot_hip.so): camera-IMU extrinsic rotation calibration of many windows on the
GPU (InitialEXRotation::CalibrationExRotation).

    eh = vio.load_exrot().create()                           # (device 0, its own stream)
    pairs = eh.relative_rotations_batch(items)               # solveRelativeR of every consecutive frame pair: one dict per window
    out = eh.calibrate_batch(items, [p["Rc"] for p in pairs])    # the recursion over the pairs from given Rc and delta_q
    out = eh.exrot_batch(items)                              # both in one call; stage 1's dict under "pairs"

An item is sfm.py's dict (n_frames F, start_frame, obs_offset, pts) plus delta_q (F - 1, 4) as (w, x, y, z): the pre-integrated rotation
between consecutive frames.  item_from_window makes one from a StreamDriver's tracks and pre-integration records.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib
from .sfm import item_from_tracks

MAX_FRAMES = 32
MAX_TRACKS = 4096
MIN_CORRES = 9
DEFAULT_MIN_FRAMES, DEFAULT_MIN_SIGMA, DEFAULT_HUBER_DEG = 10, 0.25, 5.0
OK, NOT_FINITE = 0, -3
FAIL_NOT_OBSERVABLE = 1
# StreamDriver(initialize=dict(calibrate_ric=...)): the `status` of a try whose calibration failed is TRY_FAILED_EXROT + |status| (201;
# 203 for a non-finite window), clear of sfm.TRY_FAILED_SFM's 101-103; the calibration's own status is under `exrot_status`
TRY_FAILED_EXROT = 200
STATUS_NAMES = {OK: "ok", NOT_FINITE: "not finite", FAIL_NOT_OBSERVABLE: "no step passed the gate (too few frames or too little rotation)"}


class VioExrotConfig(C.Structure):
    _fields_ = [("min_frames", C.c_int32), ("reserved", C.c_int32), ("min_sigma", C.c_double), ("huber_deg", C.c_double)]


class VioExrotItem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_tracks", C.c_int32), ("start_frame", C.c_void_p), ("obs_offset", C.c_void_p),
                ("pts", C.c_void_p), ("delta_q", C.c_void_p)]


class VioExrotPair(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_corres", C.c_int32), ("front", C.c_int32 * 4), ("choice", C.c_int32), ("det_flip", C.c_int32),
                ("Rc", C.c_double * 9)]


class VioExrotStep(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("R", C.c_double * 9), ("sigma", C.c_double * 3), ("huber", C.c_double)]


class VioExrotResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("step", C.c_int32), ("q", C.c_double * 4), ("R", C.c_double * 9)]


class ExrotLib:
    """libvio_exrot_hip.so: vio_exrot_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "relative_rotations_batch", "calibrate_batch", "batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_exrot_", self.SYMBOLS)
        self.fn["exrot_batch"] = self.fn["batch"]
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["relative_rotations_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["calibrate_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_exrot handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return ExrotHandle(self, device, stream)


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items)."""

    def __init__(self, items, tracks=True, imu=True):
        self.keep = []
        self.items = (VioExrotItem * max(1, len(items)))()
        self.np = []
        for i, it in enumerate(items):
            F = int(it["n_frames"])
            sf = off = pts = dq = None
            if tracks:
                sf = np.ascontiguousarray(it["start_frame"], dtype=np.int32)
                off = np.ascontiguousarray(it["obs_offset"], dtype=np.int64)
                pts = np.ascontiguousarray(it["pts"], dtype=np.float64).reshape(-1, 2)
                if off.size != sf.size + 1 or (off.size and off[-1] != len(pts)):
                    raise ValueError("window %d: obs_offset must have n_tracks + 1 entries and end at len(pts)" % i)
            if imu:
                dq = np.ascontiguousarray(it["delta_q"], dtype=np.float64).reshape(-1, 4)
                if len(dq) != max(F - 1, 0):
                    raise ValueError("window %d: delta_q must have n_frames - 1 rows" % i)
            self.keep += [sf, off, pts, dq]
            self.np.append(max(F - 1, 0))
            self.items[i] = VioExrotItem(F, int(sf.size) if tracks else 0, sf.ctypes.data if tracks else None,
                                         off.ctypes.data if tracks else None, pts.ctypes.data if tracks else None,
                                         dq.ctypes.data if imu else None)
        self.total = sum(self.np)
        self.base = np.concatenate([[0], np.cumsum(self.np)]).astype(np.int64)


def _pairs_dict(pairs, lo, hi):
    ps = [pairs[k] for k in range(lo, hi)]
    st = NOT_FINITE if any(p.status == NOT_FINITE for p in ps) else OK
    return dict(status=st, Rc=np.array([p.Rc[:] for p in ps]).reshape(-1, 3, 3), n_corres=np.array([p.n_corres for p in ps], dtype=np.int32),
                front=np.array([p.front[:] for p in ps], dtype=np.int32).reshape(-1, 4), choice=np.array([p.choice for p in ps], dtype=np.int32),
                det_flip=np.array([p.det_flip for p in ps], dtype=bool))


def _res_dict(r, steps, lo, hi):
    ss = [steps[k] for k in range(lo, hi)]
    return dict(status=int(r.status), step=int(r.step), q=np.array(r.q[:]), ric=np.array(r.R[:]).reshape(3, 3),
                step_q=np.array([s.q[:] for s in ss]).reshape(-1, 4), step_ric=np.array([s.R[:] for s in ss]).reshape(-1, 3, 3),
                sigma=np.array([s.sigma[:] for s in ss]).reshape(-1, 3), huber=np.array([s.huber for s in ss]))


class ExrotHandle(CompanionHandle):
    PREFIX = "vio_exrot_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_exrot_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, min_frames=DEFAULT_MIN_FRAMES, min_sigma=DEFAULT_MIN_SIGMA, huber_deg=DEFAULT_HUBER_DEG):
        cfg = VioExrotConfig(int(min_frames), 0, float(min_sigma), float(huber_deg))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def relative_rotations_batch(self, items):
        """solveRelativeR of every consecutive frame pair of every window (delta_q is not read): a list of dicts (status, Rc
        (F - 1, 3, 3), n_corres (F - 1,), front (F - 1, 4) counts for (R1, t1), (R1, t2), (R2, t1), (R2, t2), choice (F - 1,): 1 / 2 / 0
        for R1 / R2 / the identity, det_flip (F - 1,) bool).  Non-finite windows do not raise."""
        B = len(items)
        pk = _Packed(items, imu=False)
        pairs = (VioExrotPair * max(pk.total, 1))()
        st = self.lib.fn["relative_rotations_batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(pairs))
        self._ck(st, "relative_rotations_batch", allow_not_finite=True)
        return [_pairs_dict(pairs, int(pk.base[i]), int(pk.base[i + 1])) for i in range(B)]

    def calibrate_batch(self, items, Rcs):
        """The calibration recursion of every window from given pair rotations (only n_frames and delta_q of the items are read;
        Rcs[i]: (F - 1, 3, 3)): a list of dicts (status, step: the first step that passed the gate (1-based) or -1, q (w, x, y, z) and
        ric (3, 3) at that step, and per step step_q (F - 1, 4), step_ric (F - 1, 3, 3), sigma (F - 1, 3): the three smallest singular
        values, descending, huber (F - 1,): each pair's weight)."""
        B = len(items)
        pk = _Packed(items, tracks=False)
        rc = np.zeros((max(pk.total, 1), 9))
        for i in range(B):
            r = np.asarray(Rcs[i], dtype=np.float64).reshape(-1, 9)
            if len(r) != pk.np[i]:
                raise ValueError("window %d: Rc must have n_frames - 1 rotations" % i)
            rc[pk.base[i]:pk.base[i + 1]] = r
        res = (VioExrotResult * max(B, 1))()
        steps = (VioExrotStep * max(pk.total, 1))()
        st = self.lib.fn["calibrate_batch"](self.h, C.c_int32(B), C.addressof(pk.items), rc.ctypes.data, C.addressof(res), C.addressof(steps))
        self._ck(st, "calibrate_batch", allow_not_finite=True)
        return [_res_dict(res[i], steps, int(pk.base[i]), int(pk.base[i + 1])) for i in range(B)]

    def exrot_batch(self, items):
        """Both stages in one call: calibrate_batch's dicts, each with stage 1's dict under "pairs"."""
        B = len(items)
        pk = _Packed(items)
        pairs = (VioExrotPair * max(pk.total, 1))()
        res = (VioExrotResult * max(B, 1))()
        steps = (VioExrotStep * max(pk.total, 1))()
        st = self.lib.fn["batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(pairs), C.addressof(res), C.addressof(steps))
        self._ck(st, "exrot_batch", allow_not_finite=True)
        out = []
        for i in range(B):
            d = _res_dict(res[i], steps, int(pk.base[i]), int(pk.base[i + 1]))
            d["pairs"] = _pairs_dict(pairs, int(pk.base[i]), int(pk.base[i + 1]))
            out.append(d)
        return out

    def timing(self):
        """ms of the last call: host packing + upload, k_exrot_pairs, k_exrot_solve (NaN for a stage that did not run), the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "pairs_ms": t[1], "solve_ms": t[2], "total_ms": t[3]}


def delta_q_wxyz(pres):
    """delta_q (n, 4) as (w, x, y, z) of pre-integration records (theirs are stored x, y, z, w)."""
    return np.array([[p["delta_q"][3], p["delta_q"][0], p["delta_q"][1], p["delta_q"][2]] for p in pres], dtype=np.float64).reshape(-1, 4)


def item_from_window(tracks, frames, pres):
    """The calibration item of a StreamDriver's window: item_from_tracks' tracks plus the delta_q of its pre-integration records."""
    item = item_from_tracks(tracks, frames)[0]
    item["delta_q"] = delta_q_wxyz(pres)
    return item
