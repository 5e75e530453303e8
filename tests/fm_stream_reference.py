"""What include/vio_fm_stream.h's two calls are held to, over tests/fm_reference.py's track lists, and NumpyFm: a stand-in for
fm.FmHandle with its batched methods, so that a StreamDriver(features=(NumpyFm, slot)) runs without a device.

The triangulation of NumpyFm is a callable passed in, the driver's own context's `triangulate` (sf, off, pts, poses, ext, init ->
depths): fm_reference.triangulate is an SVD that is held to the device only within TRI_RTOL, and a driver compared byte for byte with
its dict path must triangulate with what that path triangulates with."""
import numpy as np

import fm_reference as fr

STATUS_CAPACITY = 4
DEPTH_SET, DEPTH_CLEAR = 0, 1


def init_depth(tracks, triangulated_depths, s):
    """visualInitialAlign's depth hand-over (estimator.cpp:406-417, :436-442): clearDepth(-1) of the usable tracks, the given
    triangulated depth (one per usable track, in list order, the < 0.1 fallback applied already), one product with s."""
    new, k = fr.copy_tracks(tracks), 0
    for t in new:
        if not fr.usable(t):
            continue
        t["depth"] = -1.0
        t["depth"] = float(np.float64(triangulated_depths[k]) * np.float64(s))
        k += 1
    assert k == len(triangulated_depths)
    return new


def tracks_arrays(tracks):
    """vio_fm_tracks_get / vio_fm_tracks_batch's arrays of a list."""
    ids, start, depth, flag, off, pts = fr.tracks_to_arrays(tracks)
    return dict(ids=ids, start=start, depth=depth, flag=flag, off=off, pts=pts.reshape(-1, 2))


WINDOW_FIELDS = ("feature_ids", "inv_depth", "lm", "host", "target", "pts_i", "pts_j")


class Recording:
    """Any handle with FmHandle's methods, every call forwarded; exports[slot] collects what each export_batch returned for the slot
    and calls the (method, number of items) of every batched call."""

    def __init__(self, handle):
        self._h, self.exports, self.calls = handle, {}, []

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if not name.endswith("_batch"):
            return fn

        def call(items, *a, **kw):
            res = fn(items, *a, **kw)
            self.calls.append((name, len(items)))
            if name == "export_batch":
                for it, r in zip(items, res):
                    self.exports.setdefault(int(it[0]), []).append({k: np.array(r[k]) for k in WINDOW_FIELDS})
            return res
        return call


def record_dict_driver(d):
    """The same record of a driver without features=: what every window_arrays call returned."""
    out, inner = [], d.window_arrays

    def window_arrays():
        w, ids = inner()
        out.append(dict(feature_ids=np.array(ids, dtype=np.int64), inv_depth=np.array(w.inv_depth), lm=np.array(w.lm), host=np.array(w.host),
                        target=np.array(w.target), pts_i=np.array(w.pts_i), pts_j=np.array(w.pts_j)))
        return w, ids
    d.window_arrays = window_arrays
    return out


class NumpyFm:
    """FmHandle's batched methods over fm_reference's functions: slot -> list of track dicts."""

    def __init__(self, triangulate, init_depth_value=fr.INIT_DEPTH):
        self.triangulate, self.init_depth_value = triangulate, init_depth_value
        self.slots = {}
        self.calls = []                                 # (method, number of items) of every batched call

    def reset(self, slot):
        self.slots[int(slot)] = []

    def counts(self, slot):
        return fr.counts(self.slots.get(int(slot), []))

    def _res(self, slot, **kw):
        r = dict(status=fr.STATUS_OK, keyframe=0, last_track_num=0, parallax_num=0, n_new=0, n_triangulated=0, n_rows=0, parallax_sum=0.0)
        r.update(zip(("n_tracks", "n_landmarks", "n_observations"), self.counts(slot)))
        r.update(kw)
        return r

    def _slots_once(self, name, slots):
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("%s: a slot is listed twice" % name)
        self.calls.append((name, len(slots)))

    def _depths(self, tracks, todo, poses, ext):
        """The triangulated depth of tracks[i], i in todo, with the < 0.1 fallback of feature_manager.cpp:251-254."""
        if not todo:
            return []
        sf, off, pts = [], [0], []
        for i in todo:
            sf.append(tracks[i]["start"]); pts.extend(tracks[i]["pts"]); off.append(off[-1] + len(tracks[i]["pts"]))
        d = self.triangulate(np.array(sf, dtype=np.int32), np.array(off, dtype=np.int64), np.array(pts).reshape(-1, 2),
                             np.ascontiguousarray(poses, dtype=np.float64), np.ascontiguousarray(ext, dtype=np.float64), -np.ones(len(todo)))
        return [float(v) for v in d]

    def add_batch(self, items):
        self._slots_once("add_batch", [it[0] for it in items])
        out = []
        for slot, fc, ids, pts in items:
            new, r = fr.add(self.slots.setdefault(int(slot), []), int(fc), ids, pts)
            self.slots[int(slot)] = new
            r.pop("parallax_sum_ref")
            out.append(self._res(slot, **r))
        return out

    def export_batch(self, items, triangulate=True):
        self._slots_once("export_batch", [it[0] for it in items])
        out = []
        for slot, poses, ext in items:
            tracks = self.slots.setdefault(int(slot), [])
            todo = [i for i, t in enumerate(tracks) if fr.usable(t) and not t["depth"] > 0] if triangulate else []
            for i, d in zip(todo, self._depths(tracks, todo, poses, ext)):
                tracks[i]["depth"] = d
            out.append(self._res(slot, n_triangulated=len(todo), **fr.export(tracks)))
        return out

    def set_depth_batch(self, items, mode=DEPTH_SET, remove_failures=False):
        self._slots_once("set_depth_batch", [it[0] for it in items])
        out = []
        for slot, x in items:
            new = fr.set_depth(self.slots[int(slot)], np.asarray(x, dtype=np.float64), clear=mode == DEPTH_CLEAR)
            self.slots[int(slot)] = fr.remove_failures(new) if remove_failures else new
            out.append(self._res(slot))
        return out

    def slide_batch(self, items):
        self._slots_once("slide_batch", [it[0] for it in items])
        out = []
        for it in items:
            slot, kind, fc = int(it[0]), int(it[1]), int(it[2]) if len(it) > 2 and it[2] is not None else 0
            mats = [np.asarray(v, dtype=np.float64) for v in it[3:7]] if kind == fr.BACK_SHIFT_DEPTH else [None] * 4
            self.slots[slot] = fr.slide(self.slots[slot], kind, fc, *mats, init_depth=self.init_depth_value)
            out.append(self._res(slot))
        return out

    def init_depth_batch(self, items):
        self._slots_once("init_depth_batch", [it[0] for it in items])
        out = []
        for slot, poses, ext, s in items:
            if not (np.isfinite(s) and s > 0):
                raise ValueError("s must be finite and > 0")
            tracks = self.slots[int(slot)]
            todo = [i for i, t in enumerate(tracks) if fr.usable(t)]
            self.slots[int(slot)] = init_depth(tracks, self._depths(tracks, todo, poses, ext), s)
            out.append(self._res(slot, n_triangulated=len(todo)))
        return out

    def tracks_get(self, slot):
        return tracks_arrays(self.slots.get(int(slot), []))

    def tracks_batch(self, slots):
        self._slots_once("tracks_batch", slots)
        out = []
        for s in slots:
            a = self.tracks_get(s)
            out.append(self._res(s, n_rows=int(a["off"][-1]), **a))
        return out
