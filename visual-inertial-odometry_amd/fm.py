"""ctypes binding of include/vio_fm.h, vio_fm_stream.h, vio_fm_outlier.h and vio_fm_predict.h (csrc/libvio_fm_hip.so): the reference's FeatureManager for many streams at once, each stream's
track list resident on the device.

    fh = vio.load_fm().create()                                      # (device 0, its own stream)
    fm = BatchFeatureManager(fh, slots=range(64))
    res = fm.add_feature_frames(bt.feature_frames(), frame_counts)   # addFeatureCheckParallax: res[i]["keyframe"]
    wins = fm.windows(poses, ext)                                    # triangulate + the arrays vio_set_landmarks / _observations take
    fm.set_depths([w["inv_depth"] for w in solved])                  # setDepth + removeFailures
    fm.remove([w["feature_ids"][flags & 7 != 0] for w, flags in zip(wins, lm_flags)])    # removeOutlier by id (vio_fm_outlier.h)
    fm.slide([BACK_SHIFT_DEPTH] * 64, marg_R=..., marg_P=..., new_R=..., new_P=...)
    pred = fm.predict(frame_count, poses, ext)                       # predictPtsInNextFrame: pred[i]["ids"], ["pts_cam"] (vio_fm_predict.h)

A track list as arrays is tests/fm_util.tracks_to_arrays' layout: ids, start, depth, flag, off (n + 1), pts (off[-1], 2).
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib

MAX_SLOTS, MAX_TRACKS, MAX_POINTS, MAX_OBS = 256, 2048, 1024, 11
DEFAULT_INIT_DEPTH, DEFAULT_MIN_PARALLAX = 5.0, 10.0 / 460.0
STATUS_OK, STATUS_TABLE_FULL, STATUS_GAP, STATUS_OBS_FULL = 0, 1, 2, 3
STATUS_CAPACITY = 4                                                    # include/vio_fm_stream.h
DEPTH_SET, DEPTH_CLEAR = 0, 1
BACK_SHIFT_DEPTH, BACK, FRONT = 0, 1, 2


class VioFmConfig(C.Structure):
    _fields_ = [("init_depth", C.c_double), ("min_parallax", C.c_double)]


class VioFmResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_tracks", C.c_int32), ("n_landmarks", C.c_int32), ("n_observations", C.c_int32),
                ("keyframe", C.c_int32), ("last_track_num", C.c_int32), ("parallax_num", C.c_int32), ("n_new", C.c_int32),
                ("n_triangulated", C.c_int32), ("n_rows", C.c_int32), ("parallax_sum", C.c_double)]


class VioFmAddItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("frame_count", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32), ("ids", C.c_void_p),
                ("pts", C.c_void_p)]


class VioFmExportItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("triangulate", C.c_int32), ("cap_landmarks", C.c_int32), ("cap_observations", C.c_int32),
                ("poses", C.c_void_p), ("ext", C.c_void_p), ("feature_ids", C.c_void_p), ("inv_depth", C.c_void_p), ("lm", C.c_void_p),
                ("host", C.c_void_p), ("target", C.c_void_p), ("pts_i", C.c_void_p), ("pts_j", C.c_void_p)]


class VioFmDepthItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("mode", C.c_int32), ("remove_failures", C.c_int32), ("n", C.c_int32), ("x", C.c_void_p)]


class VioFmSlideItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("kind", C.c_int32), ("frame_count", C.c_int32), ("reserved", C.c_int32), ("marg_R", C.c_void_p),
                ("marg_P", C.c_void_p), ("new_R", C.c_void_p), ("new_P", C.c_void_p)]


class VioFmCorrItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("l", C.c_int32), ("r", C.c_int32), ("cap_rows", C.c_int32), ("rows", C.c_void_p)]


class VioFmInitDepthItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("s", C.c_double), ("poses", C.c_void_p), ("ext", C.c_void_p)]


class VioFmTracksItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("cap_tracks", C.c_int32), ("cap_obs", C.c_int64), ("ids", C.c_void_p), ("start", C.c_void_p),
                ("depth", C.c_void_p), ("flag", C.c_void_p), ("off", C.c_void_p), ("pts", C.c_void_p)]


class VioFmRemoveItem(C.Structure):                                     # include/vio_fm_outlier.h
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("ids", C.c_void_p), ("erased", C.c_void_p)]


class VioFmPredictItem(C.Structure):                                    # include/vio_fm_predict.h
    _fields_ = [("slot", C.c_int32), ("frame_count", C.c_int32), ("cap_rows", C.c_int32), ("reserved", C.c_int32), ("poses", C.c_void_p),
                ("ext", C.c_void_p), ("next_pose", C.c_void_p), ("ids", C.c_void_p), ("pts_cam", C.c_void_p)]


def _result(r):
    return {k: getattr(r, k) for k, _ in VioFmResult._fields_}


class FmLib:
    """libvio_fm_hip.so: vio_fm_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "reset", "counts", "add_batch", "export_batch",
               "set_depth_batch", "slide_batch", "corresponding_batch", "tracks_set", "tracks_get", "timing"]
    STREAM_SYMBOLS = ["init_depth_batch", "tracks_batch"]                                  # include/vio_fm_stream.h
    OUTLIER_SYMBOLS = ["remove_batch"]                                                     # include/vio_fm_outlier.h
    PREDICT_SYMBOLS = ["predict_batch"]                                                    # include/vio_fm_predict.h

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_fm_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["reset"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["counts"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        for k in ("add_batch", "export_batch", "set_depth_batch", "slide_batch", "corresponding_batch"):
            self.fn[k].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["tracks_set"].argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        self.fn["tracks_get"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 7
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_fm_", self.STREAM_SYMBOLS)[1])
        self.fn.update(open_lib(path, "vio_fm_", self.OUTLIER_SYMBOLS)[1])
        self.fn.update(open_lib(path, "vio_fm_", self.PREDICT_SYMBOLS)[1])
        for k in self.STREAM_SYMBOLS + self.OUTLIER_SYMBOLS + self.PREDICT_SYMBOLS:
            self.fn[k].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_fm handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return FmHandle(self, device, stream)


class FmHandle(CompanionHandle):
    PREFIX = "vio_fm_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_fm_create")

    def set_config(self, init_depth=DEFAULT_INIT_DEPTH, min_parallax=DEFAULT_MIN_PARALLAX):
        cfg = VioFmConfig(float(init_depth), float(min_parallax))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def reset(self, slot):
        """clearState of one slot."""
        self._ck(self.lib.fn["reset"](self.h, C.c_int32(slot)), "reset")

    def counts(self, slot):
        """(n_tracks, n_landmarks, n_observations) of a slot as the last call left them."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.fn["counts"](self.h, C.c_int32(slot), C.byref(a), C.byref(b), C.byref(c)), "counts")
        return a.value, b.value, c.value

    def _call(self, name, items, n):
        res = (VioFmResult * max(n, 1))()
        self._ck(self.lib.fn[name](self.h, C.c_int32(n), C.addressof(items), C.addressof(res)), name)
        return [_result(res[i]) for i in range(n)]

    def add_batch(self, items):
        """addFeatureCheckParallax per item (slot, frame_count, ids (n,), pts (n, 2)): a list of result dicts (status, the three
        counts, keyframe, last_track_num, parallax_num, parallax_sum, n_new)."""
        arr, keep = (VioFmAddItem * max(len(items), 1))(), []
        for i, (slot, fc, ids, pts) in enumerate(items):
            ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
            if len(ids) != len(pts):
                raise ValueError("item %d: ids and pts must have the same length" % i)
            keep += [ids, pts]
            arr[i] = VioFmAddItem(int(slot), int(fc), len(ids), 0, ids.ctypes.data, pts.ctypes.data)
        return self._call("add_batch", arr, len(items))

    def export_batch(self, items, triangulate=True):
        """Per item (slot, poses (11, 7), ext (7,)): the result dict plus feature_ids, inv_depth, lm, host, target, pts_i, pts_j."""
        arr, keep, outs = (VioFmExportItem * max(len(items), 1))(), [], []
        for i, (slot, poses, ext) in enumerate(items):
            _, nl, no = self.counts(slot)
            poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(11, 7)
            ext = np.ascontiguousarray(ext, dtype=np.float64).reshape(7)
            o = dict(feature_ids=np.zeros(nl, dtype=np.int64), inv_depth=np.zeros(nl), lm=np.zeros(no, dtype=np.int32),
                     host=np.zeros(no, dtype=np.int32), target=np.zeros(no, dtype=np.int32), pts_i=np.zeros((no, 2)), pts_j=np.zeros((no, 2)))
            keep += [poses, ext]
            outs.append(o)
            arr[i] = VioFmExportItem(int(slot), int(bool(triangulate)), nl, no, poses.ctypes.data, ext.ctypes.data, o["feature_ids"].ctypes.data,
                                     o["inv_depth"].ctypes.data, o["lm"].ctypes.data, o["host"].ctypes.data, o["target"].ctypes.data,
                                     o["pts_i"].ctypes.data, o["pts_j"].ctypes.data)
        res = self._call("export_batch", arr, len(items))
        for r, o in zip(res, outs):
            r.update(o)
        return res

    def set_depth_batch(self, items, mode=DEPTH_SET, remove_failures=False):
        """Per item (slot, x (n_landmarks,)): setDepth (DEPTH_SET) or clearDepth (DEPTH_CLEAR), then removeFailures if asked."""
        arr, keep = (VioFmDepthItem * max(len(items), 1))(), []
        for i, (slot, x) in enumerate(items):
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            keep.append(x)
            arr[i] = VioFmDepthItem(int(slot), int(mode), int(bool(remove_failures)), x.size, x.ctypes.data)
        return self._call("set_depth_batch", arr, len(items))

    def slide_batch(self, items):
        """Per item (slot, kind, frame_count, marg_R, marg_P, new_R, new_P); the matrices are read for BACK_SHIFT_DEPTH only (None
        otherwise), frame_count for FRONT only."""
        arr, keep = (VioFmSlideItem * max(len(items), 1))(), []
        for i, it in enumerate(items):
            slot, kind, fc = int(it[0]), int(it[1]), int(it[2]) if len(it) > 2 and it[2] is not None else 0
            m = [None] * 4
            if kind == BACK_SHIFT_DEPTH:
                m = [np.ascontiguousarray(np.ravel(v), dtype=np.float64) for v in it[3:7]]
                if [v.size for v in m] != [9, 3, 9, 3]:
                    raise ValueError("item %d: marg_R (3, 3), marg_P (3,), new_R (3, 3), new_P (3,)" % i)
                keep += m
            arr[i] = VioFmSlideItem(slot, kind, fc, 0, *[None if v is None else v.ctypes.data for v in m])
        return self._call("slide_batch", arr, len(items))

    def corresponding_batch(self, items):
        """Per item (slot, l, r): the result dict plus rows (n_rows, 4) of x_l, y_l, x_r, y_r in list order."""
        arr, outs = (VioFmCorrItem * max(len(items), 1))(), []
        for i, (slot, l, r) in enumerate(items):
            n = self.counts(slot)[0]
            rows = np.zeros((n, 4))
            outs.append(rows)
            arr[i] = VioFmCorrItem(int(slot), int(l), int(r), n, rows.ctypes.data)
        res = self._call("corresponding_batch", arr, len(items))
        for r, rows in zip(res, outs):
            r["rows"] = rows[:r["n_rows"]].copy()
        return res

    def tracks_set(self, slot, ids, start, depth, flag, off, pts):
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        start = np.ascontiguousarray(start, dtype=np.int32).reshape(-1)
        depth = np.ascontiguousarray(depth, dtype=np.float64).reshape(-1)
        flag = np.ascontiguousarray(flag, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        n = len(ids)
        if not (len(start) == len(depth) == len(flag) == n and len(off) == n + 1 and (n == 0 or 0 <= off[-1] <= len(pts))):
            raise ValueError("ids, start, depth, flag need one entry per track, off one more, ending within pts")
        self._ck(self.lib.fn["tracks_set"](self.h, C.c_int32(slot), C.c_int32(n), ids.ctypes.data, start.ctypes.data, depth.ctypes.data,
                                           flag.ctypes.data, off.ctypes.data, pts.ctypes.data), "tracks_set")

    def tracks_get(self, slot):
        """The slot's list: a dict of ids, start, depth, flag, off, pts."""
        cap = self.counts(slot)[0]
        ids, start = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32)
        depth, flag = np.zeros(cap), np.zeros(cap, dtype=np.int32)
        off, pts = np.zeros(cap + 1, dtype=np.int64), np.zeros((cap * MAX_OBS, 2))
        n = C.c_int32()
        self._ck(self.lib.fn["tracks_get"](self.h, C.c_int32(slot), C.c_int32(cap), C.c_int64(cap * MAX_OBS), C.byref(n), ids.ctypes.data,
                                           start.ctypes.data, depth.ctypes.data, flag.ctypes.data, off.ctypes.data, pts.ctypes.data), "tracks_get")
        n = n.value
        return dict(ids=ids[:n], start=start[:n], depth=depth[:n], flag=flag[:n], off=off[:n + 1], pts=pts[:off[n]].copy())

    def init_depth_batch(self, items):
        """visualInitialAlign's depth hand-over per item (slot, poses (11, 7), ext (7,), s): every usable track is triangulated anew
        on the poses (the SfM's, with tic = 0 in ext) and holds that depth times s.  The result dicts; n_triangulated is the usable
        count."""
        arr, keep = (VioFmInitDepthItem * max(len(items), 1))(), []
        for i, (slot, poses, ext, s) in enumerate(items):
            poses, ext = np.ascontiguousarray(poses, dtype=np.float64), np.ascontiguousarray(ext, dtype=np.float64)
            if poses.shape != (11, 7) or ext.shape != (7,) or np.ndim(s) != 0:
                raise ValueError("item %d: poses (11, 7), ext (7,), s a scalar" % i)
            keep += [poses, ext]
            arr[i] = VioFmInitDepthItem(int(slot), 0, float(s), poses.ctypes.data, ext.ctypes.data)
        return self._call("init_depth_batch", arr, len(items))

    def tracks_batch(self, slots, cap_tracks=None, cap_obs=None):
        """The lists of `slots` in one call: per slot the dict tracks_get returns (ids, start, depth, flag, off, pts) plus the
        result's fields.  The arrays are sized from the handle's n_tracks and n_tracks * MAX_OBS (cap_tracks / cap_obs: per slot
        capacities in their place); a slot they are too small for comes back with status STATUS_CAPACITY, n_rows the observations it
        needs, and its arrays as they were allocated (zeros)."""
        slots = [int(s) for s in np.asarray(slots, dtype=np.int64).reshape(-1)]
        for name, v in (("cap_tracks", cap_tracks), ("cap_obs", cap_obs)):
            if v is not None and len(v) != len(slots):
                raise ValueError("%s: one entry per slot" % name)
        arr, outs = (VioFmTracksItem * max(len(slots), 1))(), []
        for i, slot in enumerate(slots):
            n = self.counts(slot)[0]
            ct = n if cap_tracks is None else int(cap_tracks[i])
            co = n * MAX_OBS if cap_obs is None else int(cap_obs[i])
            if ct < 0 or co < 0:
                raise ValueError("item %d: a negative capacity" % i)
            o = dict(ids=np.zeros(ct, dtype=np.int64), start=np.zeros(ct, dtype=np.int32), depth=np.zeros(ct), flag=np.zeros(ct, dtype=np.int32),
                     off=np.zeros(ct + 1, dtype=np.int64), pts=np.zeros((co, 2)))
            outs.append(o)
            arr[i] = VioFmTracksItem(slot, ct, co, o["ids"].ctypes.data, o["start"].ctypes.data, o["depth"].ctypes.data, o["flag"].ctypes.data,
                                     o["off"].ctypes.data, o["pts"].ctypes.data)
        res = self._call("tracks_batch", arr, len(slots))
        for r, o in zip(res, outs):
            if r["status"] != STATUS_OK:                 # (nothing was written: the arrays as they were allocated)
                r.update(o)
                continue
            n = r["n_tracks"]
            r.update(ids=o["ids"][:n], start=o["start"][:n], depth=o["depth"][:n], flag=o["flag"][:n], off=o["off"][:n + 1],
                     pts=o["pts"][:o["off"][n]].copy())
        return res

    def remove_batch(self, items):
        """removeOutlier by id per item (slot, ids (n,)): every row of the slot whose feature id is listed is erased, the others keep
        their order and content; an id no row has is not an error.  ids: distinct, at most MAX_TRACKS, any order (the feature_ids an
        export_batch returned).  The result dicts (the three counts after the call; n_rows: the rows erased) plus `erased`, a bool
        array in the order of ids: which of them named a row."""
        arr, keep, outs = (VioFmRemoveItem * max(len(items), 1))(), [], []
        for i, (slot, ids) in enumerate(items):
            ids = np.asarray(ids)
            if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
                raise ValueError("item %d: ids must be a one-dimensional array of integers" % i)
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if len(ids) > MAX_TRACKS:
                raise ValueError("item %d: %d ids, a slot has at most %d rows" % (i, len(ids), MAX_TRACKS))
            if len(np.unique(ids)) != len(ids):
                raise ValueError("item %d: an id is listed twice" % i)
            erased = np.zeros(len(ids), dtype=np.uint8)
            keep.append(ids)
            outs.append(erased)
            arr[i] = VioFmRemoveItem(int(slot), len(ids), ids.ctypes.data if len(ids) else None, erased.ctypes.data if len(ids) else None)
        res = self._call("remove_batch", arr, len(items))
        for r, e in zip(res, outs):
            r["erased"] = e.astype(bool)
        return res

    def predict_batch(self, items):
        """predictPtsInNextFrame per item (slot, frame_count, poses (11, 7), ext (7,), next_pose (7,) or None for the constant-velocity
        pose): the tracks with a depth that end at frame_count as points in the next frame's camera.  The result dicts (the three
        counts; n_rows: the rows predicted) plus ids (n_rows,) int64 and pts_cam (n_rows, 3) float64, in list order."""
        arr, keep, outs = (VioFmPredictItem * max(len(items), 1))(), [], []
        for i, (slot, fc, poses, ext, nxt) in enumerate(items):
            n = self.counts(slot)[0]
            poses = np.ascontiguousarray(poses, dtype=np.float64)
            ext = np.ascontiguousarray(ext, dtype=np.float64)
            nxt = None if nxt is None else np.ascontiguousarray(nxt, dtype=np.float64)
            if poses.shape != (11, 7) or ext.shape != (7,) or (nxt is not None and nxt.shape != (7,)):
                raise ValueError("item %d: poses (11, 7), ext (7,), next_pose (7,) or None" % i)
            ids, pts = np.zeros(max(n, 1), dtype=np.int64), np.zeros((max(n, 1), 3))
            keep += [poses, ext, nxt]
            outs.append((ids, pts))
            arr[i] = VioFmPredictItem(int(slot), int(fc), n, 0, poses.ctypes.data, ext.ctypes.data, None if nxt is None else nxt.ctypes.data,
                                      ids.ctypes.data, pts.ctypes.data)
        res = self._call("predict_batch", arr, len(items))
        for r, (ids, pts) in zip(res, outs):
            r.update(ids=ids[:r["n_rows"]].copy(), pts_cam=pts[:r["n_rows"]].copy())
        return res

    def timing(self):
        """ms of the last batched call that launched: host checks, packing and upload; the kernel; the read-back; the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "kernel_ms": t[1], "readback_ms": t[2], "total_ms": t[3]}


class BatchFeatureManager:
    """The reference's FeatureManager for every slot of `slots` in one call per method: the counterpart of
    frontend.BatchFeatureTracker, whose feature_frames() it takes as they are."""

    def __init__(self, handle, slots):
        self.fm, self.slots = handle, [int(s) for s in slots]
        if len(set(self.slots)) != len(self.slots):
            raise ValueError("a slot is listed twice")

    def _per_slot(self, v, what):
        v = list(v)
        if len(v) != len(self.slots):
            raise ValueError("%s: one entry per slot" % what)
        return v

    def add_feature_frames(self, frames, frame_counts):
        """frames: per slot (ids (n,), rows (n, >= 2)) with the normalised point in columns 0 and 1 (float32 widens exactly);
        frame_counts: per slot.  The result dicts of add_batch; ["keyframe"] is the marginalisation decision."""
        frames, fcs = self._per_slot(frames, "frames"), self._per_slot(frame_counts, "frame_counts")
        items = []
        for s, fc, (ids, rows) in zip(self.slots, fcs, frames):
            rows = np.asarray(rows, dtype=np.float64)
            if rows.ndim != 2 or rows.shape[0] != len(ids) or rows.shape[1] < 2:
                raise ValueError("slot %d: rows must be (len(ids), >= 2)" % s)
            items.append((s, fc, ids, rows[:, 0:2]))
        return self.fm.add_batch(items)

    def windows(self, poses, ext, triangulate=True):
        """poses: per slot (11, 7); ext: (7,) for all or per slot.  Per slot a dict of synth.Window's fields inv_depth, lm, host,
        target, pts_i, pts_j, and feature_ids, after triangulate (if asked)."""
        poses = self._per_slot(poses, "poses")
        ext = np.asarray(ext, dtype=np.float64)
        exts = [ext] * len(self.slots) if ext.ndim == 1 else self._per_slot(ext, "ext")
        return self.fm.export_batch(list(zip(self.slots, poses, exts)), triangulate=triangulate)

    def set_depths(self, inv_depths, remove_failures=True):
        """setDepth from each slot's solved inverse depths, then removeFailures."""
        return self.fm.set_depth_batch(list(zip(self.slots, self._per_slot(inv_depths, "inv_depths"))), DEPTH_SET, remove_failures)

    def clear_depths(self, inv_depths):
        return self.fm.set_depth_batch(list(zip(self.slots, self._per_slot(inv_depths, "inv_depths"))), DEPTH_CLEAR, False)

    def slide(self, kinds, frame_counts=None, marg_R=None, marg_P=None, new_R=None, new_P=None):
        """kinds: per slot BACK_SHIFT_DEPTH, BACK or FRONT; frame_counts per slot for FRONT; the four pose arrays per slot for
        BACK_SHIFT_DEPTH (entries of other slots are not read)."""
        kinds = self._per_slot(kinds, "kinds")
        n = len(self.slots)
        cols = [self._per_slot(v, "slide") if v is not None else [None] * n for v in (frame_counts, marg_R, marg_P, new_R, new_P)]
        return self.fm.slide_batch([(s, k) + tuple(c[i] for c in cols) for i, (s, k) in enumerate(zip(self.slots, kinds))])

    def corresponding(self, l, r):
        return self.fm.corresponding_batch([(s, l, r) for s in self.slots])

    def init_depths(self, poses, exts, scales):
        """visualInitialAlign's depth hand-over: poses per slot (11, 7) (the un-scaled SfM poses), exts (7,) for all or per slot (tic
        = 0), scales per slot."""
        poses, scales = self._per_slot(poses, "poses"), self._per_slot(scales, "scales")
        ext = np.asarray(exts, dtype=np.float64)
        exts = [ext] * len(self.slots) if ext.ndim == 1 else self._per_slot(ext, "exts")
        return self.fm.init_depth_batch(list(zip(self.slots, poses, exts, scales)))

    def tracks(self):
        """Every slot's list (sfm_f) in one call."""
        return self.fm.tracks_batch(self.slots)

    def predict(self, frame_count, poses, ext, next_poses=None):
        """predictPtsInNextFrame of every slot: frame_count one for all or per slot, poses per slot (11, 7), ext (7,) for all or per
        slot, next_poses None (constant velocity) or per slot (7,) / None (FmHandle.predict_batch)."""
        poses = self._per_slot(poses, "poses")
        fcs = [int(frame_count)] * len(self.slots) if np.ndim(frame_count) == 0 else self._per_slot(frame_count, "frame_count")
        ext = np.asarray(ext, dtype=np.float64)
        exts = [ext] * len(self.slots) if ext.ndim == 1 else self._per_slot(ext, "ext")
        nxt = [None] * len(self.slots) if next_poses is None else self._per_slot(next_poses, "next_poses")
        return self.fm.predict_batch(list(zip(self.slots, fcs, poses, exts, nxt)))

    def remove(self, ids_per_slot):
        """removeOutlier / removeFailures by id: per slot the feature ids whose tracks go (FmHandle.remove_batch)."""
        return self.fm.remove_batch(list(zip(self.slots, self._per_slot(ids_per_slot, "ids_per_slot"))))
