"""ctypes binding of include/vio_pnp.h (csrc/libvio_pnp_hip.so): the PnP of the non-keyframes of many windows on the GPU, the step of
Estimator::initialStructure between the SfM and the alignment (estimator.cpp:308-374).

    ph = vio.load_pnp().create()                                     # (device 0, its own stream)
    sfm = sh.sfm_batch(sfm_items)                                    # the keyframes (sfm.py)
    items = pnp_items_from_sfm(sfm, sfm_items, all_frames)           # the non-keyframes' observations against the SfM's points
    out = ph.frames_batch(items)                                     # one dict per window
    init_items = all_frames_to_init_items(sfm, out, ric, pres, is_key)      # ImageFrame::R / T of all_image_frame for InitHandle

An item is a dict: points (n_points, 3), valid (n_points,) or None, key_Q (n_key, 4) as (w, x, y, z), key_T (n_key, 3), guess_key
(n_frames,), obs_offset (n_frames + 1,), obs_point (n_obs,), obs_pts (n_obs, 2): frame k observes the points obs_point[obs_offset[k] :
obs_offset[k + 1]] at the normalised image points obs_pts[...].  Flat problems: valid = None, obs_point = arange, one key pose per frame.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib
from .sfm import quat_wxyz_to_rot

MAX_FRAMES = 32
MAX_POINTS = 4096
DEFAULT_MIN_POINTS = 6
OK, NOT_FINITE = 0, -3
FAIL_FEW_POINTS, FAIL_NO_POSE = 1, 2
STATUS_NAMES = {OK: "ok", NOT_FINITE: "not finite", FAIL_FEW_POINTS: "not enough points for solve pnp", FAIL_NO_POSE: "solve pnp fail"}


class VioPnpConfig(C.Structure):
    _fields_ = [("min_points", C.c_int32), ("reserved", C.c_int32)]


class VioPnpItem(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_key", C.c_int32), ("n_frames", C.c_int32), ("reserved", C.c_int32), ("points", C.c_void_p),
                ("valid", C.c_void_p), ("key_Q", C.c_void_p), ("key_T", C.c_void_p), ("guess_key", C.c_void_p), ("obs_offset", C.c_void_p),
                ("obs_point", C.c_void_p), ("obs_pts", C.c_void_p)]


class VioPnpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("fail_frame", C.c_int32)]


class VioPnpFrameInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_used", C.c_int32), ("reserved", C.c_int32), ("cost", C.c_double)]


class PnpLib:
    """libvio_pnp_hip.so: vio_pnp_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "frames_batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_pnp_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["frames_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_pnp handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return PnpHandle(self, device, stream)


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items).  Only the arrays' shapes are
    checked here; what they hold is the library's to check."""

    def __init__(self, items):
        self.keep = []
        self.items = (VioPnpItem * max(1, len(items)))()
        self.nf = []
        for i, it in enumerate(items):
            pts = np.ascontiguousarray(it["points"], dtype=np.float64).reshape(-1, 3)
            valid = None if it.get("valid") is None else np.ascontiguousarray(np.asarray(it["valid"]) != 0, dtype=np.uint8)
            kq = np.ascontiguousarray(it["key_Q"], dtype=np.float64).reshape(-1, 4)
            kt = np.ascontiguousarray(it["key_T"], dtype=np.float64).reshape(-1, 3)
            gk = np.ascontiguousarray(it["guess_key"], dtype=np.int32).reshape(-1)
            off = np.ascontiguousarray(it["obs_offset"], dtype=np.int64).reshape(-1)
            op = np.ascontiguousarray(it["obs_point"], dtype=np.int32).reshape(-1)
            ob = np.ascontiguousarray(it["obs_pts"], dtype=np.float64).reshape(-1, 2)
            nf = int(it.get("n_frames", len(gk)))
            if len(kq) != len(kt) or (valid is not None and len(valid) != len(pts)):
                raise ValueError("window %d: key_Q / key_T and points / valid must have the same lengths" % i)
            if len(gk) < nf or off.size != nf + 1 or len(op) != len(ob) or off[-1] != len(op):
                raise ValueError("window %d: guess_key needs n_frames entries, obs_offset n_frames + 1 ending at len(obs_point)" % i)
            self.keep += [pts, valid, kq, kt, gk, off, op, ob]
            self.nf.append(max(nf, 0))
            self.items[i] = VioPnpItem(len(pts), len(kq), nf, 0, pts.ctypes.data, None if valid is None else valid.ctypes.data,
                                       kq.ctypes.data, kt.ctypes.data, gk.ctypes.data, off.ctypes.data, op.ctypes.data, ob.ctypes.data)
        self.total = sum(self.nf)
        self.base = np.concatenate([[0], np.cumsum(self.nf)]).astype(np.int64)


class PnpHandle(CompanionHandle):
    PREFIX = "vio_pnp_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_pnp_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, min_points=DEFAULT_MIN_POINTS):
        cfg = VioPnpConfig(int(min_points), 0)
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def frames_batch(self, items):
        """The PnP of every non-keyframe of every window: a list of dicts (status, fail_frame: the first failing frame or -1, Q
        (n_frames, 4) wxyz and T (n_frames, 3): R_pnp / T_pnp of estimator.cpp:365-371 in vio_sfm_result's convention, NaN for a frame
        that failed, and per frame frame_status, iterations, n_used, cost).  Non-finite windows do not raise."""
        B = len(items)
        pk = _Packed(items)
        res = (VioPnpResult * max(B, 1))()
        Q = np.full((max(pk.total, 1), 4), np.nan)
        T = np.full((max(pk.total, 1), 3), np.nan)
        info = (VioPnpFrameInfo * max(pk.total, 1))()
        st = self.lib.fn["frames_batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(res), Q.ctypes.data, T.ctypes.data,
                                         C.addressof(info))
        self._ck(st, "frames_batch", allow_not_finite=True)
        out = []
        for i in range(B):
            lo, hi = int(pk.base[i]), int(pk.base[i + 1])
            fi = [info[k] for k in range(lo, hi)]
            out.append(dict(status=int(res[i].status), fail_frame=int(res[i].fail_frame), Q=Q[lo:hi].copy(), T=T[lo:hi].copy(),
                            frame_status=np.array([f.status for f in fi], dtype=np.int32),
                            iterations=np.array([f.iterations for f in fi], dtype=np.int32),
                            n_used=np.array([f.n_used for f in fi], dtype=np.int32), cost=np.array([f.cost for f in fi], dtype=np.float64)))
        return out

    def timing(self):
        """ms of the last call that launched: host packing + upload, k_pnp_frames, the whole call."""
        t = (C.c_double * 3)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "total_ms": t[2]}


def guess_keys(is_key):
    """The keyframe whose pose is each non-keyframe's guess (estimator.cpp:312-327): the next keyframe in time order.  is_key: one
    flag per frame of all_image_frame in time order; the first and the last frame must be keyframes."""
    key = [bool(k) for k in is_key]
    if not key or not key[0] or not key[-1]:
        raise ValueError("the first and the last frame of all_image_frame must be keyframes")
    out, i = [], 0
    for k in key:
        if k:
            i += 1
        else:
            out.append(i)
    return np.array(out, dtype=np.int32)


def pnp_items_from_sfm(sfm_results, sfm_items, all_frames):
    """The PnP items of SfM results.  sfm_results: sfm_batch's dicts; sfm_items: the items they came from; all_frames[i]:
    all_image_frame of window i in time order, one dict per frame: is_key, and for a non-keyframe obs_point (the SfM item's track of
    each observation) and obs_pts (n, 2).  The keyframes of all_frames[i] are the SfM item's frames, in order; the first and the last
    frame must be keyframes (ValueError otherwise).  A window whose SfM did not succeed gives an item without frames."""
    out = []
    for i, (r, item, frames) in enumerate(zip(sfm_results, sfm_items, all_frames)):
        key = [bool(f["is_key"]) for f in frames]
        gk = guess_keys(key)
        if sum(key) != int(item["n_frames"]):
            raise ValueError("window %d: all_frames has %d keyframes, the SfM item %d frames" % (i, sum(key), int(item["n_frames"])))
        nt = len(item["start_frame"])
        if r["status"] != OK:
            out.append(dict(points=np.zeros((0, 3)), valid=None, key_Q=np.zeros((0, 4)), key_T=np.zeros((0, 3)),
                            guess_key=np.zeros(0, dtype=np.int32), obs_offset=np.zeros(1, dtype=np.int64),
                            obs_point=np.zeros(0, dtype=np.int32), obs_pts=np.zeros((0, 2))))
            continue
        off, op, ob = [0], [], []
        for f in frames:
            if f["is_key"]:
                continue
            p = np.asarray(f["obs_point"], dtype=np.int32).reshape(-1)
            if p.size and (p.min() < 0 or p.max() >= nt):
                raise ValueError("window %d: an observation's track is outside the SfM item" % i)
            op.append(p)
            ob.append(np.asarray(f["obs_pts"], dtype=np.float64).reshape(-1, 2))
            off.append(off[-1] + p.size)
        out.append(dict(points=np.asarray(r["points"], dtype=np.float64), valid=np.asarray(r["state"], dtype=bool),
                        key_Q=np.asarray(r["Q"], dtype=np.float64), key_T=np.asarray(r["T"], dtype=np.float64), guess_key=gk,
                        obs_offset=np.array(off, dtype=np.int64),
                        obs_point=np.concatenate(op) if op else np.zeros(0, dtype=np.int32),
                        obs_pts=np.concatenate(ob) if ob else np.zeros((0, 2))))
    return out


def all_frames_to_init_items(sfm_results, pnp_results, ric, pres, is_key):
    """The alignment items of all_image_frame as initialStructure leaves it (estimator.cpp:316-318, 365-372): R = Q RIC^T and T of every
    frame in time order, the keyframes' from the SfM and the others' from the PnP, with is_key set.  ric: RIC[0] (3 x 3); pres[i]: the
    pre-integration records between consecutive frames of window i's all_image_frame; is_key[i]: its flags.  A window whose SfM or
    PnP did not succeed gives None.  Without non-keyframes this is sfm_items_to_init_items' result."""
    ric = np.asarray(ric, dtype=np.float64).reshape(3, 3)
    out = []
    for i, (s, p) in enumerate(zip(sfm_results, pnp_results)):
        key = np.array([bool(k) for k in is_key[i]])
        if s["status"] != OK or (p is not None and p["status"] != OK):
            out.append(None)
            continue
        nk, nn = int(key.sum()), int((~key).sum())
        if nk != len(s["Q"]) or nn != (0 if p is None else len(p["Q"])):
            raise ValueError("window %d: is_key does not match the SfM's keyframes and the PnP's frames" % i)
        Q, T = np.zeros((len(key), 4)), np.zeros((len(key), 3))
        Q[key], T[key] = s["Q"], s["T"]
        if nn:
            Q[~key], T[~key] = p["Q"], p["T"]
        R = np.stack([quat_wxyz_to_rot(q) @ ric.T for q in Q])
        out.append(dict(R=R, T=T, pre=list(pres[i]), is_key=[int(k) for k in key]))
    return out
