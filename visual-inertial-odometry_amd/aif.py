"""ctypes binding of include/vio_aif.h (csrc/libvio_aif_hip.so): the reference Estimator's all_image_frame and tmp_pre_integration for
many streams at once, each stream's map resident on the device.

    ah = vio.load_aif().create()                                     # (device 0, its own stream)
    frames = BatchImageFrames(ah, slots=range(64))
    frames.process_imu(runs)                                         # processIMU's part over each slot's (dt (n,), acc (n, 3), gyr (n, 3))
    frames.image(headers, ids, pts, ba, bg)                          # processImage's insert: the frame takes the open interval
    frames.slide(t_0)                                                # slideWindow's erase of every frame with header <= t_0
    out = frames.structure(items)                                    # initialStructure's frame work: records, excitation, key walk, PnP, R / T
    recs = frames.propagate(ba, bg)                                  # per slot the records of its frames' intervals at the given biases

A slot as a dict is tests/aif_reference.py's layout: frames (a list of dicts t, ids, pts, R, T, is_key, exists, first, bias, dt, acc,
gyr), open (the open interval: exists, first, bias, dt, acc, gyr), acc_0, gyr_0, first_imu.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, VioPreint, open_lib
from .pnp import VioPnpFrameInfo

MAX_SLOTS, MAX_FRAMES, MAX_FRAME_POINTS, MAX_POINTS, MAX_SAMPLES, OFFS = 256, 32, 1024, 8192, 4096, 34
STATUS_OK, STATUS_POOL_FULL, STATUS_FRAMES_FULL, STATUS_NO_FRAME, STATUS_WALK = 0, 1, 2, 3, 4
MAX_KEY, MAX_TRACKS = 32, 4096
DEFAULT_NOISE = (0.2687, 0.2121, 7.07e-6, 7.07e-7)
DEFAULT_MIN_POINTS = 6


class VioAifConfig(C.Structure):
    _fields_ = [("noise", C.c_double * 4), ("min_points", C.c_int32), ("reserved", C.c_int32)]


class VioAifResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_samples", C.c_int32),
                ("erased_frames", C.c_int32), ("erased_samples", C.c_int32), ("records", C.c_int32), ("reserved", C.c_int32)]


class VioAifImuItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("dt", C.c_void_p), ("acc", C.c_void_p), ("gyr", C.c_void_p)]


class VioAifImageItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("t", C.c_double), ("ids", C.c_void_p), ("pts", C.c_void_p), ("ba", C.c_double * 3),
                ("bg", C.c_double * 3)]


class VioAifSlideItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("t_0", C.c_double)]


class VioAifPropagateItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("ba", C.c_double * 3), ("bg", C.c_double * 3), ("pre", C.c_void_p)]


class VioAifStructureItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_key", C.c_int32), ("n_tracks", C.c_int32), ("reserved", C.c_int32), ("headers", C.c_void_p),
                ("Q", C.c_void_p), ("T", C.c_void_p), ("track_ids", C.c_void_p), ("points", C.c_void_p), ("state", C.c_void_p),
                ("ric", C.c_double * 9), ("R", C.c_void_p), ("T_out", C.c_void_p), ("is_key", C.c_void_p), ("pre", C.c_void_p),
                ("frame_info", C.c_void_p)]


class VioAifStructureResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("pnp_status", C.c_int32), ("fail_frame", C.c_int32), ("n_frames", C.c_int32), ("n_key", C.c_int32),
                ("low_excitation", C.c_int32), ("var", C.c_double)]


class VioAifSlot(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("first_imu", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32),
                ("exists", C.c_int32 * OFFS), ("is_key", C.c_int32 * MAX_FRAMES), ("pt_off", C.c_int32 * OFFS), ("samp_off", C.c_int64 * OFFS),
                ("t", C.c_double * MAX_FRAMES), ("R", C.c_double * (9 * MAX_FRAMES)), ("T", C.c_double * (3 * MAX_FRAMES)),
                ("first", C.c_double * (6 * OFFS)), ("bias", C.c_double * (6 * OFFS)), ("acc_0", C.c_double * 3), ("gyr_0", C.c_double * 3)]


def _result(r):
    return {k: getattr(r, k) for k, _ in VioAifResult._fields_[:7]}


def slot_to_dict(s, ids, pts, dt, acc, gyr):
    """A downloaded VioAifSlot and its pools as the slot dict of the module's docstring."""
    F = int(s.n_frames)
    po, so = np.array(s.pt_off, dtype=np.int64), np.array(s.samp_off, dtype=np.int64)
    first, bias = np.array(s.first).reshape(OFFS, 6), np.array(s.bias).reshape(OFFS, 6)
    R, T = np.array(s.R).reshape(MAX_FRAMES, 9), np.array(s.T).reshape(MAX_FRAMES, 3)

    def interval(j):
        a, b = int(so[j]), int(so[j + 1])
        return dict(exists=int(s.exists[j]), first=first[j].copy(), bias=bias[j].copy(), dt=dt[a:b].copy(), acc=acc[a:b].copy(), gyr=gyr[a:b].copy())

    frames = []
    for j in range(F):
        a, b = int(po[j]), int(po[j + 1])
        f = dict(t=float(s.t[j]), ids=ids[a:b].copy(), pts=pts[a:b].copy(), R=R[j].copy(), T=T[j].copy(), is_key=int(s.is_key[j]))
        f.update(interval(j))
        frames.append(f)
    return dict(frames=frames, open=interval(F), acc_0=np.array(s.acc_0), gyr_0=np.array(s.gyr_0), first_imu=int(s.first_imu))


class AifLib:
    """libvio_aif_hip.so: vio_aif_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "reset", "imu_batch", "image_batch", "slide_batch",
               "propagate_batch", "structure_batch", "frames_get", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_aif_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["reset"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["frames_get"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        for k in ("imu_batch", "image_batch", "slide_batch", "propagate_batch", "structure_batch"):
            self.fn[k].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_aif handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return AifHandle(self, device, stream)


class AifHandle(CompanionHandle):
    PREFIX = "vio_aif_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_aif_create")
        self.noise = tuple(DEFAULT_NOISE)          # what the handle propagates with: the library's default until set_config

    def set_config(self, noise=DEFAULT_NOISE, min_points=DEFAULT_MIN_POINTS):
        """The IMU noise (acc_n, gyr_n, acc_w, gyr_w, or a dict of them) and the PnP's min_points."""
        if isinstance(noise, dict):
            noise = [noise[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")]
        nz = np.asarray(noise, dtype=np.float64).reshape(-1)
        if nz.size != 4:
            raise ValueError("noise (4,)")
        cfg = VioAifConfig((C.c_double * 4)(*nz), int(min_points), 0)
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")
        self.noise = tuple(float(v) for v in nz)

    def reset(self, slot):
        """clearState of one slot: the map and the open interval go, acc_0 / gyr_0 stay."""
        self._ck(self.lib.fn["reset"](self.h, C.c_int32(slot)), "reset")

    def frames_get(self, slot):
        """The slot as a dict (the module's docstring)."""
        s = VioAifSlot()
        ids, pts = np.zeros(MAX_POINTS, dtype=np.int64), np.zeros((MAX_POINTS, 2))
        dt, acc, gyr = np.zeros(MAX_SAMPLES), np.zeros((MAX_SAMPLES, 3)), np.zeros((MAX_SAMPLES, 3))
        self._ck(self.lib.fn["frames_get"](self.h, C.c_int32(slot), C.addressof(s), C.c_int64(MAX_POINTS), ids.ctypes.data, pts.ctypes.data,
                                           C.c_int64(MAX_SAMPLES), dt.ctypes.data, acc.ctypes.data, gyr.ctypes.data), "frames_get")
        return slot_to_dict(s, ids, pts, dt, acc, gyr)

    def _call(self, name, items, n):
        res = (VioAifResult * max(n, 1))()
        self._ck(self.lib.fn[name](self.h, C.c_int32(n), C.addressof(items), C.addressof(res)), name)
        return [_result(res[i]) for i in range(n)]

    def imu_batch(self, items):
        """processIMU's part per item (slot, dt (n,), acc (n, 3), gyr (n, 3)): result dicts (status, n_frames, n_points, n_samples)."""
        arr, keep = (VioAifImuItem * max(len(items), 1))(), []
        for i, (slot, dt, acc, gyr) in enumerate(items):
            dt = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
            acc = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 3)
            gyr = np.ascontiguousarray(gyr, dtype=np.float64).reshape(-1, 3)
            if not len(dt) == len(acc) == len(gyr):
                raise ValueError("item %d: dt, acc and gyr must have the same length" % i)
            keep += [dt, acc, gyr]
            ptr = lambda a: a.ctypes.data if a.size else None
            arr[i] = VioAifImuItem(int(slot), len(dt), ptr(dt), ptr(acc), ptr(gyr))
        return self._call("imu_batch", arr, len(items))

    def image_batch(self, items):
        """processImage's insert per item (slot, t, ids (n,), pts (n, 2), ba (3,), bg (3,))."""
        arr, keep = (VioAifImageItem * max(len(items), 1))(), []
        for i, (slot, t, ids, pts, ba, bg) in enumerate(items):
            ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
            ba, bg = np.asarray(ba, dtype=np.float64).reshape(-1), np.asarray(bg, dtype=np.float64).reshape(-1)
            if len(ids) != len(pts) or ba.size != 3 or bg.size != 3:
                raise ValueError("item %d: ids (n,), pts (n, 2), ba (3,), bg (3,)" % i)
            keep += [ids, pts]
            ptr = lambda a: a.ctypes.data if a.size else None
            arr[i] = VioAifImageItem(int(slot), len(ids), float(t), ptr(ids), ptr(pts), (C.c_double * 3)(*ba), (C.c_double * 3)(*bg))
        return self._call("image_batch", arr, len(items))

    def slide_batch(self, items):
        """slideWindow's erase per item (slot, t_0): result dicts (status, erased_frames, erased_samples, ...)."""
        arr = (VioAifSlideItem * max(len(items), 1))()
        for i, (slot, t_0) in enumerate(items):
            arr[i] = VioAifSlideItem(int(slot), 0, float(t_0))
        return self._call("slide_batch", arr, len(items))

    def propagate_batch(self, items):
        """Per item (slot, ba (3,), bg (3,)): the result dict plus preint, a (VioPreint * 31) whose first `records` entries are the
        slot's intervals 1 .. n_frames - 1 at those biases."""
        arr, outs = (VioAifPropagateItem * max(len(items), 1))(), []
        for i, (slot, ba, bg) in enumerate(items):
            ba, bg = np.asarray(ba, dtype=np.float64).reshape(-1), np.asarray(bg, dtype=np.float64).reshape(-1)
            if ba.size != 3 or bg.size != 3:
                raise ValueError("item %d: ba (3,), bg (3,)" % i)
            out = (VioPreint * (MAX_FRAMES - 1))()
            outs.append(out)
            arr[i] = VioAifPropagateItem(int(slot), 0, (C.c_double * 3)(*ba), (C.c_double * 3)(*bg), C.addressof(out))
        res = self._call("propagate_batch", arr, len(items))
        for r, o in zip(res, outs):
            r["preint"] = o
        return res

    def structure_batch(self, items):
        """initialStructure's frame work per item, a dict: slot, headers (n_key,), Q (n_key, 4) wxyz and T (n_key, 3) of the SfM, track_ids
        (n_tracks,), points (n_tracks, 3), state (n_tracks,), ric (3, 3).  Per item a dict: status, pnp_status, fail_frame, n_frames,
        n_key, low_excitation, var, and for the slot's F frames R (F, 3, 3), T (F, 3), is_key (F,), frame_status, iterations, n_used,
        cost (F,), and preint, a (VioPreint * 31) whose first F - 1 entries are the frames' records at their constructor biases."""
        n = len(items)
        arr, keep, outs = (VioAifStructureItem * max(n, 1))(), [], []
        for i, it in enumerate(items):
            hd = np.ascontiguousarray(it["headers"], dtype=np.float64).reshape(-1)
            Q = np.ascontiguousarray(it["Q"], dtype=np.float64).reshape(-1, 4)
            T = np.ascontiguousarray(it["T"], dtype=np.float64).reshape(-1, 3)
            ids = np.ascontiguousarray(it["track_ids"], dtype=np.int64).reshape(-1)
            pts = np.ascontiguousarray(it["points"], dtype=np.float64).reshape(-1, 3)
            state = np.ascontiguousarray(np.asarray(it["state"]) != 0, dtype=np.uint8).reshape(-1)
            ric = np.ascontiguousarray(it["ric"], dtype=np.float64).reshape(-1)
            if not (len(hd) == len(Q) == len(T) and len(ids) == len(pts) == len(state) and ric.size == 9):
                raise ValueError("item %d: headers / Q / T need n_key rows, track_ids / points / state n_tracks, ric (3, 3)" % i)
            o = dict(R=np.full((MAX_FRAMES, 9), np.nan), T=np.full((MAX_FRAMES, 3), np.nan), is_key=np.zeros(MAX_FRAMES, dtype=np.uint8),
                     preint=(VioPreint * (MAX_FRAMES - 1))(), info=(VioPnpFrameInfo * MAX_FRAMES)())
            keep += [hd, Q, T, ids, pts, state]
            outs.append(o)
            ptr = lambda a: a.ctypes.data if a.size else None
            arr[i] = VioAifStructureItem(int(it["slot"]), len(hd), len(ids), 0, ptr(hd), ptr(Q), ptr(T), ptr(ids), ptr(pts), ptr(state),
                                         (C.c_double * 9)(*ric), o["R"].ctypes.data, o["T"].ctypes.data, o["is_key"].ctypes.data,
                                         C.addressof(o["preint"]), C.addressof(o["info"]))
        res = (VioAifStructureResult * max(n, 1))()
        self._ck(self.lib.fn["structure_batch"](self.h, C.c_int32(n), C.addressof(arr), C.addressof(res)), "structure_batch")
        out = []
        for r, o in zip(res, outs):
            F = int(r.n_frames)
            fi = [o["info"][k] for k in range(F)]
            d = {k: getattr(r, k) for k, _ in VioAifStructureResult._fields_}
            d.update(R=o["R"][:F].reshape(F, 3, 3).copy(), T=o["T"][:F].copy(), is_key=o["is_key"][:F].copy(), preint=o["preint"],
                     frame_status=np.array([f.status for f in fi], dtype=np.int32), iterations=np.array([f.iterations for f in fi], dtype=np.int32),
                     n_used=np.array([f.n_used for f in fi], dtype=np.int32), cost=np.array([f.cost for f in fi], dtype=np.float64))
            out.append(d)
        return out

    def timing(self):
        """ms of the last batched call that launched: host checks, packing and upload; the kernels; the read-back; the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "readback_ms": t[2], "total_ms": t[3]}


class BatchImageFrames:
    """all_image_frame for every slot of `slots` in one call per method: the counterpart of est.BatchEstimatorState.  `handle` is an
    AifHandle, or anything with its batched methods (tests/aif_reference.py's ImageFramesReference)."""

    def __init__(self, handle, slots):
        self.aif, self.slots = handle, [int(s) for s in slots]
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
        return self.aif.imu_batch(items)

    def image(self, headers, ids, pts, ba=None, bg=None):
        """Per slot the header, the feature ids (n,) and points (n, 2) of its image, and Bas / Bgs[frame_count] (default 0)."""
        n = len(self.slots)
        ba = [np.zeros(3)] * n if ba is None else self._per_slot(ba, "ba")
        bg = [np.zeros(3)] * n if bg is None else self._per_slot(bg, "bg")
        return self.aif.image_batch(list(zip(self.slots, self._per_slot(headers, "headers"), self._per_slot(ids, "ids"), self._per_slot(pts, "pts"), ba, bg)))

    def slide(self, t_0):
        """t_0: per slot the header of the window's oldest frame (Headers[0] before the slide)."""
        return self.aif.slide_batch(list(zip(self.slots, self._per_slot(t_0, "t_0"))))

    def structure(self, items):
        """items: per slot a dict headers, Q, T, track_ids, points, state, ric (AifHandle.structure_batch's, without the slot)."""
        return self.aif.structure_batch([dict(it, slot=s) for s, it in zip(self.slots, self._per_slot(items, "items"))])

    def propagate(self, ba, bg):
        """Per slot the records of intervals 1 .. n_frames - 1 at biases ba, bg ((3,) for every slot, or one per slot)."""
        n = len(self.slots)
        ba, bg = np.asarray(ba, dtype=np.float64), np.asarray(bg, dtype=np.float64)
        ba, bg = np.broadcast_to(ba, (n, 3)), np.broadcast_to(bg, (n, 3))
        return self.aif.propagate_batch([(s, ba[i], bg[i]) for i, s in enumerate(self.slots)])


def initialize_from_frames(frames, init_handle, sfm_results, headers, track_ids, ric, tic, g_norm):
    """One INITIAL try of every slot of `frames` (a BatchImageFrames) from its resident all_image_frame, in four calls for the whole
    batch: structure, vio_init_gyro_bias_batch on its R / T and records, propagate at (0, bg), vio_init_align_batch.  sfm_results[i]:
    slot i's SfM (sfm_batch's or construct_batch's dict: status, Q, T, points, state); headers[i]: its Headers[]; track_ids[i]: the
    feature ids of the SfM item's tracks; ric: RIC (3, 3), one for all or one per slot; init_handle: an InitHandle.  Returns what
    InitHandle.initialize_batch returns, with `structure` (the structure call's dict) added; None for a slot whose SfM, key walk or
    PnP did not succeed."""
    from .init import NOT_FINITE, OK
    from .imu import record_dict
    n = len(frames.slots)
    ric = np.asarray(ric, dtype=np.float64)
    ric = np.broadcast_to(ric.reshape(-1, 3, 3), (n, 3, 3))
    live = [i for i in range(n) if sfm_results[i]["status"] == OK]
    out = [None] * n
    if not live:
        return out
    sub = BatchImageFrames(frames.aif, [frames.slots[i] for i in live])
    st = sub.structure([dict(headers=headers[i], Q=sfm_results[i]["Q"], T=sfm_results[i]["T"], track_ids=track_ids[i],
                             points=sfm_results[i]["points"], state=sfm_results[i]["state"], ric=ric[i]) for i in live])
    good = [k for k, o in enumerate(st) if o["status"] == STATUS_OK and o["pnp_status"] == OK]
    if not good:
        return out
    sub = BatchImageFrames(frames.aif, [sub.slots[k] for k in good])
    items = [dict(R=st[k]["R"], T=st[k]["T"], pre=[st[k]["preint"][j] for j in range(st[k]["n_frames"] - 1)], is_key=st[k]["is_key"]) for k in good]
    bg, gst = init_handle.gyro_bias_batch(items, status=True)
    bg0 = np.nan_to_num(bg, nan=0.0)
    rec = sub.propagate(np.zeros(3), bg0)
    pres = [[r["preint"][j] for j in range(r["records"])] for r in rec]
    res = init_handle.align_batch([dict(it, pre=pres[k]) for k, it in enumerate(items)], tic, g_norm, bg0)
    for k, o in enumerate(res):
        o["bg"] = bg[k].copy()
        o["pre"] = [record_dict(r) for r in pres[k]]
        o["structure"] = st[good[k]]
        if gst[k] != OK:               # as InitHandle.initialize_batch: nothing after a failed gyro step holds
            o["status"] = NOT_FINITE
            for key in ("s", "s_linear"):
                o[key] = np.nan
            for key in ("g", "g_world", "g_linear", "rot", "x", "poses", "speed_bias"):
                o[key] = np.full_like(o[key], np.nan)
        out[live[good[k]]] = o
    return out
