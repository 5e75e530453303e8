"""ctypes binding of include/vio_est.h (csrc/libvio_est_hip.so): the reference's Estimator window state and IMU buffers for many
streams at once, each stream's state resident on the device.

    eh = vio.load_est().create()                                     # (device 0, its own stream)
    eh.set_config(tic, ric_quat, g, noise)
    est = BatchEstimatorState(eh, slots=range(64))
    est.process_imu(runs)                                            # processIMU over each slot's (dt (n,), acc (n, 3), gyr (n, 3))
    est.image(headers, advance=True)                                 # Headers[frame_count] = header, frame_count++
    wins = est.windows()                                             # vector2double + the ten pre-integrations per slot
    res = est.update(poses, speed_bias, ext)                         # double2vector + failureDetection: res[i]["failure"]
    out = est.slide(kinds)                                           # slideWindow; out["marg_R"], ... go to BatchFeatureManager.slide
    est.init_apply(poses, speed_bias, g, rot)                        # visualInitialAlign's writes (include/vio_est_init.h)
    res = est.relinearize(ba_thresh, bg_thresh)                      # repropagate where a bias moved: res[i]["n_relinearized"], ["mask"]

A slot's state as a dict is tests/est_reference.py's layout: the fields of VioEstState as arrays, plus off (12,), dt, acc, gyr.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, VioPreint, open_lib

MAX_SLOTS, MAX_SAMPLES, WINDOW_SIZE, FRAMES = 256, 4096, 10, 11
STATUS_OK, STATUS_POOL_FULL, STATUS_NOT_READY = 0, 1, 2
MARG_OLD, MARG_SECOND_NEW = 0, 1
GATE_NONE, GATE_BA, GATE_BG, GATE_TRANSLATION, GATE_Z = 0, 1, 2, 3, 4
DEFAULT_G = (0.0, 0.0, 9.81)
DEFAULT_NOISE = (0.2687, 0.2121, 7.07e-6, 7.07e-7)


class VioEstConfig(C.Structure):
    _fields_ = [("tic", C.c_double * 3), ("ric", C.c_double * 4), ("g", C.c_double * 3), ("noise", C.c_double * 4)]


class VioEstState(C.Structure):
    _fields_ = [("frame_count", C.c_int32), ("first_imu", C.c_int32), ("failure_occur", C.c_int32), ("reserved", C.c_int32),
                ("exists", C.c_int32 * 12), ("Ps", C.c_double * 33), ("Rs", C.c_double * 99), ("Vs", C.c_double * 33),
                ("Bas", C.c_double * 33), ("Bgs", C.c_double * 33), ("Headers", C.c_double * 11), ("tic", C.c_double * 3),
                ("ric", C.c_double * 9), ("g", C.c_double * 3), ("acc_0", C.c_double * 3), ("gyr_0", C.c_double * 3),
                ("first", C.c_double * 66), ("lin_bias", C.c_double * 66), ("last_R", C.c_double * 9), ("last_P", C.c_double * 3),
                ("last_R0", C.c_double * 9), ("last_P0", C.c_double * 3)]


# the array fields of a state dict and their shapes
STATE_ARRAYS = dict(Ps=(11, 3), Rs=(11, 9), Vs=(11, 3), Bas=(11, 3), Bgs=(11, 3), Headers=(11,), tic=(3,), ric=(9,), g=(3,), acc_0=(3,),
                    gyr_0=(3,), first=(11, 6), lin_bias=(11, 6), last_R=(9,), last_P=(3,), last_R0=(9,), last_P0=(3,))
STATE_INTS = ("frame_count", "first_imu", "failure_occur")


class VioEstResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("frame_count", C.c_int32), ("n_samples", C.c_int32), ("failure", C.c_int32), ("gate", C.c_int32),
                ("singular", C.c_int32), ("slid", C.c_int32), ("shift_depth", C.c_int32), ("marg_R", C.c_double * 9),
                ("marg_P", C.c_double * 3), ("new_R", C.c_double * 9), ("new_P", C.c_double * 3)]


class VioEstImuItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("dt", C.c_void_p), ("acc", C.c_void_p), ("gyr", C.c_void_p)]


class VioEstImageItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("advance", C.c_int32), ("header", C.c_double)]


class VioEstWindowItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("poses", C.c_void_p), ("speed_bias", C.c_void_p), ("ext", C.c_void_p),
                ("preint", C.c_void_p)]


class VioEstUpdateItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("commit_last", C.c_int32), ("poses", C.c_void_p), ("speed_bias", C.c_void_p), ("ext", C.c_void_p),
                ("poses_out", C.c_void_p), ("speed_bias_out", C.c_void_p), ("ext_out", C.c_void_p)]


class VioEstSlideItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("kind", C.c_int32), ("nonlinear", C.c_int32), ("reserved", C.c_int32)]


class VioEstInitItem(C.Structure):
    """include/vio_est_init.h"""
    _fields_ = [("slot", C.c_int32), ("commit_last", C.c_int32), ("poses", C.c_double * 77), ("speed_bias", C.c_double * 99), ("g", C.c_double * 3),
                ("rot", C.c_double * 9)]


class VioEstRelinItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("ba_thresh", C.c_double), ("bg_thresh", C.c_double)]


class VioEstRelinResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("frame_count", C.c_int32), ("n_relinearized", C.c_int32), ("mask", C.c_int32)]


def _result(r):
    out = {k: getattr(r, k) for k, _ in VioEstResult._fields_[:8]}
    out.update(marg_R=np.array(r.marg_R).reshape(3, 3), marg_P=np.array(r.marg_P), new_R=np.array(r.new_R).reshape(3, 3), new_P=np.array(r.new_P))
    return out


def state_to_struct(state):
    """A state dict (the scalar and array fields; exists (11,) or (12,)) as a VioEstState."""
    s = VioEstState()
    for k in STATE_INTS:
        setattr(s, k, int(state[k]))
    ex = np.zeros(12, dtype=np.int32)
    e = np.asarray(state["exists"], dtype=np.int32).reshape(-1)
    if e.size not in (11, 12):
        raise ValueError("exists: 11 entries")
    ex[:e.size] = e
    s.exists = (C.c_int32 * 12)(*ex.tolist())
    for k, shape in STATE_ARRAYS.items():
        v = np.ascontiguousarray(state[k], dtype=np.float64)
        if v.size != int(np.prod(shape)):
            raise ValueError("%s: shape %s" % (k, shape))
        C.memmove(C.addressof(getattr(s, k)), v.ctypes.data, v.nbytes)
    return s


def struct_to_state(s):
    out = {k: int(getattr(s, k)) for k in STATE_INTS}
    out["exists"] = np.array(s.exists, dtype=np.int32)[:11].copy()
    for k, shape in STATE_ARRAYS.items():
        out[k] = np.array(getattr(s, k), dtype=np.float64).reshape(shape)
    return out


class EstLib:
    """libvio_est_hip.so: vio_est_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "reset", "state_set", "state_get", "imu_batch", "image_batch",
               "window_batch", "update_batch", "slide_batch", "timing"]
    INIT_SYMBOLS = ["init_apply_batch", "relinearize_batch"]                               # include/vio_est_init.h

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_est_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["reset"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["state_set"].argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
        self.fn["state_get"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        self.fn.update(open_lib(path, "vio_est_", self.INIT_SYMBOLS)[1])
        for k in ["imu_batch", "image_batch", "window_batch", "update_batch", "slide_batch"] + self.INIT_SYMBOLS:
            self.fn[k].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_est handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return EstHandle(self, device, stream)


class EstHandle(CompanionHandle):
    PREFIX = "vio_est_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_est_create")

    def set_config(self, tic=(0.0, 0.0, 0.0), ric=(0.0, 0.0, 0.0, 1.0), g=DEFAULT_G, noise=DEFAULT_NOISE):
        """setParameter's inputs (ric: quaternion x, y, z, w) and the IMU noise (acc_n, gyr_n, acc_w, gyr_w, or a dict of them)."""
        if isinstance(noise, dict):
            noise = [noise[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")]
        vals = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (tic, ric, g, noise)]
        if [v.size for v in vals] != [3, 4, 3, 4]:
            raise ValueError("tic (3,), ric (4,), g (3,), noise (4,)")
        cfg = VioEstConfig((C.c_double * 3)(*vals[0]), (C.c_double * 4)(*vals[1]), (C.c_double * 3)(*vals[2]), (C.c_double * 4)(*vals[3]))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def reset(self, slot):
        """clearState + setParameter of one slot."""
        self._ck(self.lib.fn["reset"](self.h, C.c_int32(slot)), "reset")

    def state_set(self, slot, state):
        """Seed one slot from a state dict (samples: off (12,), dt (S,), acc (S, 3), gyr (S, 3); absent: no samples)."""
        s = state_to_struct(state)
        off = np.ascontiguousarray(state.get("off", np.zeros(12)), dtype=np.int64).reshape(-1)
        if off.size != 12:
            raise ValueError("off: 12 entries")
        S = int(off[-1])
        dt = np.ascontiguousarray(state.get("dt", np.zeros(0)), dtype=np.float64).reshape(-1)
        acc = np.ascontiguousarray(state.get("acc", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        gyr = np.ascontiguousarray(state.get("gyr", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        if not (0 <= S <= len(dt) and len(acc) == len(dt) == len(gyr)):
            raise ValueError("dt, acc, gyr need off[11] samples")
        ptr = lambda a: a.ctypes.data if a.size else None
        self._ck(self.lib.fn["state_set"](self.h, C.c_int32(slot), C.addressof(s), off.ctypes.data, ptr(dt), ptr(acc), ptr(gyr)), "state_set")

    def state_get(self, slot):
        """The slot's whole state as a dict."""
        s, off = VioEstState(), np.zeros(12, dtype=np.int64)
        dt, acc, gyr = np.zeros(MAX_SAMPLES), np.zeros((MAX_SAMPLES, 3)), np.zeros((MAX_SAMPLES, 3))
        self._ck(self.lib.fn["state_get"](self.h, C.c_int32(slot), C.addressof(s), C.c_int64(MAX_SAMPLES), off.ctypes.data, dt.ctypes.data,
                                          acc.ctypes.data, gyr.ctypes.data), "state_get")
        out = struct_to_state(s)
        S = int(off[-1])
        out.update(off=off, dt=dt[:S].copy(), acc=acc[:S].copy(), gyr=gyr[:S].copy())
        return out

    def _call(self, name, items, n):
        res = (VioEstResult * max(n, 1))()
        self._ck(self.lib.fn[name](self.h, C.c_int32(n), C.addressof(items), C.addressof(res)), name)
        return [_result(res[i]) for i in range(n)]

    def imu_batch(self, items):
        """processIMU per item (slot, dt (n,), acc (n, 3), gyr (n, 3)): result dicts (status, frame_count, n_samples)."""
        arr, keep = (VioEstImuItem * max(len(items), 1))(), []
        for i, (slot, dt, acc, gyr) in enumerate(items):
            dt = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
            acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 3)
            gyr = np.ascontiguousarray(gyr, dtype=np.float64).reshape(-1, 3)
            if not len(dt) == len(acc) == len(gyr):
                raise ValueError("item %d: dt, acc and gyr must have the same length" % i)
            keep += [dt, acc, gyr]
            ptr = lambda a: a.ctypes.data if a.size else None
            arr[i] = VioEstImuItem(int(slot), len(dt), ptr(dt), ptr(acc), ptr(gyr))
        return self._call("imu_batch", arr, len(items))

    def image_batch(self, items):
        """Per item (slot, header, advance): Headers[frame_count] = header, frame_count++ if advance and frame_count < 10."""
        arr = (VioEstImageItem * max(len(items), 1))()
        for i, (slot, header, advance) in enumerate(items):
            arr[i] = VioEstImageItem(int(slot), int(bool(advance)), float(header))
        return self._call("image_batch", arr, len(items))

    def window_batch(self, slots):
        """Per slot: the result dict plus poses (11, 7), speed_bias (11, 9), ext (7,) and preint, a (VioPreint * 10)."""
        arr, outs = (VioEstWindowItem * max(len(slots), 1))(), []
        for i, slot in enumerate(slots):
            o = dict(poses=np.zeros((11, 7)), speed_bias=np.zeros((11, 9)), ext=np.zeros(7), preint=(VioPreint * 10)())
            outs.append(o)
            arr[i] = VioEstWindowItem(int(slot), 0, o["poses"].ctypes.data, o["speed_bias"].ctypes.data, o["ext"].ctypes.data, C.addressof(o["preint"]))
        res = self._call("window_batch", arr, len(slots))
        for r, o in zip(res, outs):
            r.update(o)
        return res

    def update_batch(self, items):
        """double2vector + failureDetection per item (slot, poses (11, 7), speed_bias (11, 9), ext (7,), commit_last): the result dict
        (failure, gate, singular) plus poses, speed_bias, ext: vector2double of the updated state."""
        arr, keep, outs = (VioEstUpdateItem * max(len(items), 1))(), [], []
        for i, (slot, poses, sb, ext, commit) in enumerate(items):
            poses = np.ascontiguousarray(poses, dtype=np.float64)
            sb = np.ascontiguousarray(sb, dtype=np.float64)
            ext = np.ascontiguousarray(ext, dtype=np.float64)
            if (poses.shape, sb.shape, ext.shape) != ((11, 7), (11, 9), (7,)):
                raise ValueError("item %d: poses (11, 7), speed_bias (11, 9), ext (7,)" % i)
            keep += [poses, sb, ext]
            o = dict(poses=np.zeros((11, 7)), speed_bias=np.zeros((11, 9)), ext=np.zeros(7))
            outs.append(o)
            arr[i] = VioEstUpdateItem(int(slot), int(bool(commit)), poses.ctypes.data, sb.ctypes.data, ext.ctypes.data, o["poses"].ctypes.data,
                                      o["speed_bias"].ctypes.data, o["ext"].ctypes.data)
        res = self._call("update_batch", arr, len(items))
        for r, o in zip(res, outs):
            r.update(o)
        return res

    def slide_batch(self, items):
        """slideWindow per item (slot, kind, nonlinear): result dicts (slid, shift_depth, marg_R, marg_P, new_R, new_P)."""
        arr = (VioEstSlideItem * max(len(items), 1))()
        for i, (slot, kind, nonlinear) in enumerate(items):
            arr[i] = VioEstSlideItem(int(slot), int(kind), int(bool(nonlinear)), 0)
        return self._call("slide_batch", arr, len(items))

    def init_apply_batch(self, items):
        """visualInitialAlign's writes per item (slot, poses (11, 7), speed_bias (11, 9), g (3,), rot (3, 3)[, commit_last]): the rows and
        the result fields of a successful alignment; commit_last (default False) also sets last_R / last_P / last_R0 / last_P0 from the
        window written.  Result dicts (status: STATUS_NOT_READY where the window is not full or an interval is missing, and the slot is
        as it was)."""
        arr = (VioEstInitItem * max(len(items), 1))()
        for i, (slot, poses, sb, g, rot, *commit) in enumerate(items):
            vals = [np.ascontiguousarray(v, dtype=np.float64) for v in (poses, sb, g, rot)]
            if [v.size for v in vals] != [77, 99, 3, 9] or vals[0].shape != (11, 7) or vals[1].shape != (11, 9):
                raise ValueError("item %d: poses (11, 7), speed_bias (11, 9), g (3,), rot (3, 3)" % i)
            if not all(np.isfinite(v).all() for v in vals):
                raise ValueError("item %d: a non-finite entry (a failed alignment's rows are NaN: list the successes only)" % i)
            arr[i].slot, arr[i].commit_last = int(slot), int(bool(commit[0])) if commit else 0
            for k, v in zip(("poses", "speed_bias", "g", "rot"), vals):
                C.memmove(C.addressof(getattr(arr[i], k)), v.ctypes.data, v.nbytes)
        return self._call("init_apply_batch", arr, len(items))

    def relinearize_batch(self, items):
        """repropagate per item (slot, ba_thresh, bg_thresh) for the intervals whose start frame's bias moved past a threshold: dicts
        (status, frame_count, n_relinearized, mask: bit j for interval j)."""
        arr = (VioEstRelinItem * max(len(items), 1))()
        for i, (slot, tba, tbg) in enumerate(items):
            tba, tbg = float(tba), float(tbg)
            if not (np.isfinite(tba) and np.isfinite(tbg) and tba >= 0.0 and tbg >= 0.0):
                raise ValueError("item %d: thresholds are finite and >= 0" % i)
            arr[i] = VioEstRelinItem(int(slot), 0, tba, tbg)
        n = len(items)
        res = (VioEstRelinResult * max(n, 1))()
        self._ck(self.lib.fn["relinearize_batch"](self.h, C.c_int32(n), C.addressof(arr), C.addressof(res)), "relinearize_batch")
        return [{k: int(getattr(res[i], k)) for k, _ in VioEstRelinResult._fields_} for i in range(n)]

    def timing(self):
        """ms of the last batched call that launched: host checks, packing and upload; the kernels; the read-back; the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "readback_ms": t[2], "total_ms": t[3]}


class BatchEstimatorState:
    """The reference's Estimator state for every slot of `slots` in one call per method: the counterpart of fm.BatchFeatureManager.
    `handle` is an EstHandle, or anything with its batched methods (tests/est_reference.py's EstimatorReference)."""

    def __init__(self, handle, slots):
        self.est, self.slots = handle, [int(s) for s in slots]
        if len(set(self.slots)) != len(self.slots):
            raise ValueError("a slot is listed twice")

    def _per_slot(self, v, what):
        v = list(v)
        if len(v) != len(self.slots):
            raise ValueError("%s: one entry per slot" % what)
        return v

    def process_imu(self, runs):
        """runs: per slot (dt (n,), acc (n, 3), gyr (n, 3)), or an interval dict with those keys."""
        items = []
        for s, r in zip(self.slots, self._per_slot(runs, "runs")):
            dt, acc, gyr = (r["dt"], r["acc"], r["gyr"]) if isinstance(r, dict) else r
            items.append((s, dt, acc, gyr))
        return self.est.imu_batch(items)

    def image(self, headers, advance=True):
        headers = self._per_slot(headers, "headers")
        adv = [advance] * len(self.slots) if isinstance(advance, (bool, int)) else self._per_slot(advance, "advance")
        return self.est.image_batch(list(zip(self.slots, headers, adv)))

    def windows(self):
        """Per slot poses, speed_bias, ext as vio_set_window takes them and preint, the ten records vio_set_imu_all takes."""
        return self.est.window_batch(self.slots)

    def update(self, poses, speed_bias, ext, commit_last=True):
        """double2vector from each slot's solved arrays, then failureDetection: per slot failure, gate, singular."""
        poses, sb, ext = self._per_slot(poses, "poses"), self._per_slot(speed_bias, "speed_bias"), self._per_slot(ext, "ext")
        return self.est.update_batch([(s, p, b, e, commit_last) for s, p, b, e in zip(self.slots, poses, sb, ext)])

    def slide(self, kinds, nonlinear=True):
        """kinds: per slot MARG_OLD or MARG_SECOND_NEW.  A dict: results (per slot), and marg_R, marg_P, new_R, new_P per slot, what
        BatchFeatureManager.slide takes for the slots that slid the old way."""
        res = self.est.slide_batch([(s, k, nonlinear) for s, k in zip(self.slots, self._per_slot(kinds, "kinds"))])
        return dict(results=res, marg_R=[r["marg_R"] for r in res], marg_P=[r["marg_P"] for r in res], new_R=[r["new_R"] for r in res],
                    new_P=[r["new_P"] for r in res])

    def init_apply(self, poses, speed_bias, g, rot, commit_last=False):
        """visualInitialAlign's writes from each slot's alignment result (its poses, speed_bias, g and rot); commit_last: also
        last_R / last_P / last_R0 / last_P0 from the window written."""
        cols = [self._per_slot(v, k) for v, k in ((poses, "poses"), (speed_bias, "speed_bias"), (g, "g"), (rot, "rot"))]
        return self.est.init_apply_batch([(s,) + tuple(c) + (commit_last,) for s, *c in zip(self.slots, *cols)])

    def relinearize(self, ba_thresh, bg_thresh):
        """repropagate, per slot, the intervals whose start frame's bias moved past the thresholds (scalars, or one per slot)."""
        ta = [ba_thresh] * len(self.slots) if np.isscalar(ba_thresh) else self._per_slot(ba_thresh, "ba_thresh")
        tg = [bg_thresh] * len(self.slots) if np.isscalar(bg_thresh) else self._per_slot(bg_thresh, "bg_thresh")
        return self.est.relinearize_batch(list(zip(self.slots, ta, tg)))
