"""ctypes binding of include/vio_frame.h (csrc/libvio_frame_hip.so): frames that stay on the GPU across CLAHE, tracking and detection,
the image steps of FeatureTracker::readImage (feature_tracker.cpp:87-149) for many image streams without the four uploads per frame.

    fr = vio.load_frame().create()                                   # (device 0, its own stream)
    fr.set_config(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow=dict(levels=4), detect=dict(min_distance=30))
    fr.push(img)                                                     # slot 0: upload once, equalise, build the pyramid; does not wait
    fr.push(img2)                                                    # the former frame is `prev` now
    out = fr.track(prev_pts)                                         # FlowHandle.track's dict, from prev into next
    out = fr.detect(tracked=pts, track_cnt=cnt, max_total=150)       # DetectHandle.detect's dict, on next
    fr.set_mask(mask, slot=0); fr.download(slot=0, which=NEXT, level=0); fr.counters(); fr.reset(slot=0)
    fr.push_batch([dict(slot=s, img=a), ...]); fr.track_batch([dict(slot=s, prev_pts=p, guess=None), ...])
    fr.detect_batch([dict(slot=s, tracked=p, track_cnt=c, max_total=150), ...])

    fr.set_camera(fx=, fy=, cx=, cy=, k1=, k2=, p1=, p2=, width=, height=); fr.set_tracker(max_cnt=150, border=1)
    outs = fr.read_batch(imgs, times, slots=[0, 1, ...], publish=True)    # all of readImage and updateID per slot, the points resident:
                                                                     # dicts of pts, ids, track_cnt, un_pts, velocity, n_new, ...
    fr.points_set(pts, ids, track_cnt, slot=0); fr.points_get(slot=0)

    fr.set_slot_camera(3, model=camera.MODEL_KANNALA_BRANDT, width=752, height=480, k2=.., mu=.., mv=.., u0=.., v0=..)   # slot 3's own camera
    fr.set_slot_camera(4, **camera.parse_camodocal_yaml(text)); fr.clear_slot_camera(4); fr.slot_camera(3)               # (include/vio_frame_camera.h)
    fr.set_reject_config(seed=0, ransac_hypotheses=128); fr.read_lift_info(3)                 # dict(n_clamped, n_bad) of slot 3's last read

    fr.set_flow_back(levels=2, max_dist=0.5); fr.track(prev_pts, back=True)                   # the forward-backward check (include/vio_frame_back.h)
    fr.set_reject_with_f(False); fr.read_back_info(0)                                          # no rejectWithF in a published read; the check's counts

    fr.set_prediction_batch([(slot, ids, pixels), ...]); fr.set_prediction_fallback(10)         # predicted pixels for the next read_batch's
    fr.clear_prediction(slot); fr.read_predict_info(slot)                                      # tracking step (include/vio_frame_predict.h)

A handle is what frontend.FeatureTracker takes as `frames`, and what frontend.BatchFeatureTracker drives through read_batch.
"""
import ctypes as C

import numpy as np

from .camera import MAX_PARAMS, PARAMS, VioCameraModel, model_params
from .capi import CompanionHandle, VioError, open_lib
from .clahe import DEFAULT_CLIP_LIMIT, DEFAULT_TILES, VioClaheConfig
from .detect import DEFAULT_MAX_TOTAL, DEFAULT_MIN_DISTANCE, DEFAULT_QUALITY, VioDetectConfig, VioDetectResult
from .reject import DEFAULT_F_THRESHOLD, DEFAULT_FOCAL_LENGTH, DEFAULT_HYPOTHESES, MODEL_PINHOLE, VioRejectCamera, VioRejectConfig
from .flow import (DEFAULT_BACK_MAX_DIST, DEFAULT_BORDER, DEFAULT_HALF_PATCH, DEFAULT_LEVELS, DEFAULT_MAX_ITER, VioFlowBackConfig, VioFlowBackInfo,
                   VioFlowConfig, VioFlowPtInfo, _image, track_results)

MAX_SLOTS, MAX_DIM = 256, 16384
PREV, NEXT = 0, 1
MAX_TRACK_POINTS, DEFAULT_MAX_CNT, DEFAULT_TRACK_BORDER = 1024, 150, 1
OK, NOT_FINITE = 0, -3


class VioFramePushItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("img", C.c_void_p)]


class VioFrameTrackItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_pts", C.c_int32), ("prev_pts", C.c_void_p), ("guess", C.c_void_p)]


class VioFrameDetectItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_tracked", C.c_int32), ("max_total", C.c_int32), ("reserved", C.c_int32), ("tracked", C.c_void_p),
                ("track_cnt", C.c_void_p), ("keep_order", C.c_void_p), ("new_pts", C.c_void_p)]


class VioFrameReadItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("img", C.c_void_p),
                ("time", C.c_double), ("pts", C.c_void_p), ("ids", C.c_void_p), ("track_cnt", C.c_void_p), ("un_pts", C.c_void_p),
                ("velocity", C.c_void_p)]


class VioFrameReadResult(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("status", "n", "n_new", "n_tracked_in", "n_after_track", "n_after_reject", "reject_status",
                                         "reject_hyp", "n_candidates", "reserved")]


class VioFramePredictionItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("ids", C.c_void_p), ("pixels", C.c_void_p)]


class FrameLib:
    """libvio_frame_hip.so: vio_frame_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "push_batch", "track_batch", "set_mask", "detect_batch",
               "download", "reset", "counters", "timing"]
    READ_SYMBOLS = ["set_camera", "set_tracker", "read_batch", "points_set", "points_get", "read_timing"]      # include/vio_frame_read.h
    CAMERA_SYMBOLS = ["set_slot_camera", "get_slot_camera", "set_reject_config", "read_lift_info"]            # include/vio_frame_camera.h
    BACK_SYMBOLS = ["set_flow_back", "track_back_batch", "set_reject_with_f", "read_back_info"]                # include/vio_frame_back.h
    PREDICT_SYMBOLS = ["set_prediction_batch", "clear_prediction", "set_prediction_fallback", "read_predict_info"]   # include/vio_frame_predict.h

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_frame_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["push_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self.fn["track_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["set_mask"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        self.fn["detect_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["download"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self.fn["reset"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["counters"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_frame_", self.READ_SYMBOLS)[1])
        self.fn["set_camera"].argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["set_tracker"].argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        self.fn["read_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        self.fn["points_set"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["points_get"].argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
        self.fn["read_timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_frame_", self.CAMERA_SYMBOLS)[1])
        self.fn["set_slot_camera"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self.fn["get_slot_camera"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_reject_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["read_lift_info"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_frame_", self.BACK_SYMBOLS)[1])
        self.fn["set_flow_back"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["track_back_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["set_reject_with_f"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["read_back_info"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_frame_", self.PREDICT_SYMBOLS)[1])
        self.fn["set_prediction_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self.fn["clear_prediction"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["set_prediction_fallback"].argtypes = [C.c_void_p, C.c_int32]
        self.fn["read_predict_info"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_frame handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return FrameHandle(self, device, stream)


class FrameHandle(CompanionHandle):
    PREFIX = "vio_frame_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        self.levels = DEFAULT_LEVELS
        self.shapes = {}                    # slot -> (height, width) of its resident frames
        self._cfg = dict(equalize=False, clahe={}, flow={}, detect={})
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_frame_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, equalize=None, clahe=None, flow=None, detect=None):
        """equalize: bool; clahe: dict(clip_limit, tiles=(tiles_x, tiles_y)); flow: dict of FlowHandle.set_config's arguments; detect:
        dict(quality, min_distance).  An argument left None keeps what the handle has; a dict replaces that library's settings (what
        it does not name returns to the default).  A change of flow's levels drops every resident frame."""
        new = dict(self._cfg)
        for k, v in (("equalize", equalize), ("clahe", clahe), ("flow", flow), ("detect", detect)):
            if v is not None:
                new[k] = bool(v) if k == "equalize" else dict(v)
        c, f, d = new["clahe"], new["flow"], new["detect"]
        tiles = c.get("tiles", (DEFAULT_TILES, DEFAULT_TILES))
        cc = VioClaheConfig(float(c.get("clip_limit", DEFAULT_CLIP_LIMIT)), int(tiles[0]), int(tiles[1]))
        fc = VioFlowConfig(int(f.get("levels", DEFAULT_LEVELS)), int(f.get("half_patch", DEFAULT_HALF_PATCH)), int(f.get("max_iter", DEFAULT_MAX_ITER)),
                           int(f.get("inverse", 0)), int(f.get("border", DEFAULT_BORDER)), int(f.get("early_stop", 0)))
        dc = VioDetectConfig(float(d.get("quality", DEFAULT_QUALITY)), int(d.get("min_distance", DEFAULT_MIN_DISTANCE)), 0)
        self._ck(self.lib.fn["set_config"](self.h, C.c_int32(1 if new["equalize"] else 0), C.byref(cc), C.byref(fc), C.byref(dc)), "set_config")
        self._cfg = new
        if fc.levels != self.levels:
            self.shapes = {}
        self.levels = fc.levels

    # ---- frames ---------------------------------------------------------------------------
    def push_batch(self, items):
        """items: dicts of slot and img ((height, width) uint8, rows may be strided).  Each becomes its slot's `next`.  Does not wait."""
        B = len(items)
        arr = (VioFramePushItem * max(B, 1))()
        keep = []
        for i, it in enumerate(items):
            a = _image(it["img"])
            keep.append(a)
            arr[i] = VioFramePushItem(int(it.get("slot", 0)), a.shape[1], a.shape[0], a.strides[0], a.ctypes.data)
        self._ck(self.lib.fn["push_batch"](self.h, C.c_int32(B), C.addressof(arr)), "push_batch")
        for i, it in enumerate(items):
            self.shapes[int(it.get("slot", 0))] = keep[i].shape

    def push(self, img, slot=0):
        self.push_batch([dict(slot=slot, img=img)])

    def reset(self, slot=0):
        """Drop the slot's frames (its mask stays): the next push may bring another geometry."""
        self._ck(self.lib.fn["reset"](self.h, C.c_int32(slot)), "reset")
        self.shapes.pop(int(slot), None)

    def set_mask(self, mask, slot=0):
        """The slot's mask, like its images, zero where nothing may be detected; None clears it."""
        if mask is None:
            self._ck(self.lib.fn["set_mask"](self.h, C.c_int32(slot), None, 0, 0, 0), "set_mask")
            return
        m = _image(mask)
        self._ck(self.lib.fn["set_mask"](self.h, C.c_int32(slot), m.ctypes.data, C.c_int32(m.shape[1]), C.c_int32(m.shape[0]),
                                         C.c_int32(m.strides[0])), "set_mask")

    def download(self, slot=0, which=NEXT, level=0):
        """Level `level` of the slot's prev (PREV) or next (NEXT): a uint8 array.  It waits for the device."""
        shape = self.shapes.get(int(slot))
        if shape is None or not 0 <= int(level) < self.levels:
            out = np.zeros(1, dtype=np.uint8)           # (the library says what is wrong)
            self._ck(self.lib.fn["download"](self.h, C.c_int32(slot), C.c_int32(which), C.c_int32(level), out.ctypes.data), "download")
            raise VioError(-1, "vio_frame_download", "the binding does not know the slot's geometry")
        h, w = shape[0] >> int(level), shape[1] >> int(level)
        out = np.zeros((h, w), dtype=np.uint8)
        self._ck(self.lib.fn["download"](self.h, C.c_int32(slot), C.c_int32(which), C.c_int32(level), out.ctypes.data), "download")
        return out

    # ---- tracking -------------------------------------------------------------------------
    def set_flow_back(self, enabled=True, levels=0, max_dist=DEFAULT_BACK_MAX_DIST):
        """FlowHandle.set_back for the handle's tracker: track, track_batch and read_batch apply the forward-backward check."""
        cfg = VioFlowBackConfig(1 if enabled else 0, int(levels), float(max_dist))
        self._ck(self.lib.fn["set_flow_back"](self.h, C.byref(cfg)), "set_flow_back")

    def track_batch(self, items, back=False):
        """items: dicts of slot, prev_pts (n, 2) float32, guess (n, 2) or None.  FlowHandle.track_batch's list of dicts (back=True: with
        the check's rows; the check must be on)."""
        B = len(items)
        arr = (VioFrameTrackItem * max(B, 1))()
        keep, n = [], []
        for i, it in enumerate(items):
            pts = np.ascontiguousarray(it["prev_pts"], dtype=np.float32).reshape(-1, 2)
            g = None if it.get("guess") is None else np.ascontiguousarray(it["guess"], dtype=np.float32).reshape(-1, 2)
            if g is not None and len(g) != len(pts):
                raise ValueError("item %d: guess needs one row per keypoint" % i)
            k = int(it.get("n_pts", len(pts)))
            keep += [pts, g]
            n.append(max(k, 0))
            arr[i] = VioFrameTrackItem(int(it.get("slot", 0)), k, pts.ctypes.data, None if g is None else g.ctypes.data)
        total = sum(n)
        base = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        nxt = np.full((max(total, 1), 2), np.nan, dtype=np.float32)
        info = (VioFlowPtInfo * max(total, 1))()
        binfo = None
        if back:
            binfo = (VioFlowBackInfo * max(total, 1))()
            st = self.lib.fn["track_back_batch"](self.h, C.c_int32(B), C.addressof(arr), nxt.ctypes.data, C.addressof(info), C.addressof(binfo))
        else:
            st = self.lib.fn["track_batch"](self.h, C.c_int32(B), C.addressof(arr), nxt.ctypes.data, C.addressof(info))
        self._ck(st, "track_back_batch" if back else "track_batch", allow_not_finite=True)
        return track_results(base, nxt, info, binfo)

    def track(self, prev_pts, guess=None, slot=0, back=False):
        return self.track_batch([dict(slot=slot, prev_pts=prev_pts, guess=guess)], back=back)[0]

    # ---- detection ------------------------------------------------------------------------
    def detect_batch(self, items):
        """items: dicts of slot, tracked (n, 2) float32 or None, track_cnt (n,) int32, max_total.  DetectHandle.detect_batch's list of
        dicts.  The mask is the slot's (set_mask)."""
        B = len(items)
        arr = (VioFrameDetectItem * max(B, 1))()
        res = (VioDetectResult * max(B, 1))()
        keep, kos, npts = [], [], []
        for i, it in enumerate(items):
            trk = it.get("tracked")
            pts = np.zeros((0, 2), dtype=np.float32) if trk is None else np.ascontiguousarray(trk, dtype=np.float32).reshape(-1, 2)
            cnt = it.get("track_cnt")
            cnt = np.ones(len(pts), dtype=np.int32) if cnt is None else np.ascontiguousarray(cnt, dtype=np.int32).reshape(-1)
            if len(cnt) != len(pts):
                raise ValueError("item %d: track_cnt needs one entry per tracked point" % i)
            max_total = int(it.get("max_total", DEFAULT_MAX_TOTAL))
            ko = np.full(max(len(pts), 1), -1, dtype=np.int32)
            npt = np.full((max(max_total, 1), 2), np.nan, dtype=np.float32)
            keep += [pts, cnt]
            kos.append(ko)
            npts.append(npt)
            arr[i] = VioFrameDetectItem(int(it.get("slot", 0)), len(pts), max_total, 0, pts.ctypes.data, cnt.ctypes.data, ko.ctypes.data,
                                        npt.ctypes.data)
        st = self.lib.fn["detect_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res))
        self._ck(st, "detect_batch", allow_not_finite=True)
        out = []
        for i in range(B):
            r = res[i]
            out.append(dict(status=int(r.status), n_kept=int(r.n_kept), n_new=int(r.n_new), n_candidates=int(r.n_candidates),
                            max_response=float(r.max_response), keep_order=kos[i][:r.n_kept].copy(), new_pts=npts[i][:r.n_new].copy()))
        return out

    def detect(self, tracked=None, track_cnt=None, max_total=DEFAULT_MAX_TOTAL, slot=0):
        return self.detect_batch([dict(slot=slot, tracked=tracked, track_cnt=track_cnt, max_total=max_total)])[0]

    # ---- readImage on resident points ------------------------------------------------------
    def set_camera(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, width=752, height=480, model=MODEL_PINHOLE, seed=0,
                   ransac_hypotheses=DEFAULT_HYPOTHESES, f_threshold=DEFAULT_F_THRESHOLD, focal_length=DEFAULT_FOCAL_LENGTH):
        """The camera of RejectHandle.set_camera and the settings of RejectHandle.set_config, for read_batch."""
        cam = VioRejectCamera(float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(p1), float(p2), int(width), int(height),
                              int(model), 0)
        cfg = VioRejectConfig(int(seed) & 0xFFFFFFFF, int(ransac_hypotheses), float(f_threshold), float(focal_length))
        self._ck(self.lib.fn["set_camera"](self.h, C.byref(cam), C.byref(cfg)), "set_camera")

    def set_slot_camera(self, slot, model=MODEL_PINHOLE, width=752, height=480, **params):
        """The slot's own camera, of any model of camera.PARAMS, by camera.model_params' keywords (camera.parse_camodocal_yaml's dict goes
        straight in).  A refused camera raises and leaves the slot as it was."""
        p = model_params(int(model), **params)
        cam = VioCameraModel(int(model), int(width), int(height), 0, (C.c_double * MAX_PARAMS)(*(p + [0.0] * (MAX_PARAMS - len(p)))))
        self._ck(self.lib.fn["set_slot_camera"](self.h, C.c_int32(int(slot)), C.byref(cam)), "set_slot_camera")

    def clear_slot_camera(self, slot):
        """The slot lifts through the handle's camera (set_camera) again."""
        self._ck(self.lib.fn["set_slot_camera"](self.h, C.c_int32(int(slot)), None), "set_slot_camera")

    def slot_camera(self, slot):
        """None, or set_slot_camera's keywords of the slot's own camera."""
        on, cam = C.c_int32(0), VioCameraModel()
        self._ck(self.lib.fn["get_slot_camera"](self.h, C.c_int32(int(slot)), C.addressof(on), C.addressof(cam)), "get_slot_camera")
        if not on.value:
            return None
        out = dict(model=int(cam.model), width=int(cam.width), height=int(cam.height))
        out.update({name: float(cam.params[i]) for i, (name, _) in enumerate(PARAMS[int(cam.model)])})
        return out

    def set_reject_config(self, seed=0, ransac_hypotheses=DEFAULT_HYPOTHESES, f_threshold=DEFAULT_F_THRESHOLD, focal_length=DEFAULT_FOCAL_LENGTH):
        """RejectHandle.set_config's settings for read_batch, without a handle-wide camera."""
        cfg = VioRejectConfig(int(seed) & 0xFFFFFFFF, int(ransac_hypotheses), float(f_threshold), float(focal_length))
        self._ck(self.lib.fn["set_reject_config"](self.h, C.byref(cfg)), "set_reject_config")

    def read_lift_info(self, slot=0):
        """dict(n_clamped, n_bad) of the undistortedPoints stage of the slot's last read_batch."""
        c, b = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.fn["read_lift_info"](self.h, C.c_int32(int(slot)), C.addressof(c), C.addressof(b)), "read_lift_info")
        return dict(n_clamped=int(c.value), n_bad=int(b.value))

    def set_reject_with_f(self, enabled=True):
        """False: a published read_batch runs no rejectWithF (n_after_reject = n_after_track, reject_hyp -1); the default is True."""
        self._ck(self.lib.fn["set_reject_with_f"](self.h, C.c_int32(1 if enabled else 0)), "set_reject_with_f")

    def read_back_info(self, slot=0):
        """dict(n_checked, n_back_lost, n_back_far) of the forward-backward check in the slot's last read_batch (zeros with it off)."""
        c, l, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.fn["read_back_info"](self.h, C.c_int32(int(slot)), C.addressof(c), C.addressof(l), C.addressof(f)), "read_back_info")
        return dict(n_checked=int(c.value), n_back_lost=int(l.value), n_back_far=int(f.value))

    def set_prediction_batch(self, items):
        """items: (slot, ids (n,), pixels (n, 2)) each: the pixels the tracks `ids` are expected at in the slot's next image
        (frontend.predict_pixels_batch).  The next read_batch that lists the slot starts those points' search there and every other
        point's at its own pixel; the prediction is used by that one read.  It replaces the slot's pending prediction; nothing is
        stored if an item is refused (a pixel that is not finite, more than MAX_TRACK_POINTS rows, a slot listed twice)."""
        B = len(items)
        arr = (VioFramePredictionItem * max(B, 1))()
        keep = []
        for i, (slot, ids, pixels) in enumerate(items):
            d = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            p = np.ascontiguousarray(pixels, dtype=np.float32).reshape(-1, 2)
            if len(d) != len(p):
                raise ValueError("item %d: ids and pixels must have the same length" % i)
            keep += [d, p]
            arr[i] = VioFramePredictionItem(int(slot), len(d), d.ctypes.data, p.ctypes.data)
        self._ck(self.lib.fn["set_prediction_batch"](self.h, C.c_int32(B), C.addressof(arr)), "set_prediction_batch")

    def clear_prediction(self, slot=0):
        """Drops the slot's pending prediction, if it has one."""
        self._ck(self.lib.fn["clear_prediction"](self.h, C.c_int32(int(slot))), "clear_prediction")

    def set_prediction_fallback(self, min_tracked=0):
        """VINS-Fusion's fallback: a slot whose guessed pass leaves fewer than min_tracked points with status 0 is tracked again without
        a guess, on the device.  0, the default: never."""
        self._ck(self.lib.fn["set_prediction_fallback"](self.h, C.c_int32(int(min_tracked))), "set_prediction_fallback")

    def read_predict_info(self, slot=0):
        """dict(n_listed, n_guessed, n_ok_guessed, fell_back) of the prediction in the slot's last read_batch (zeros without one)."""
        v = [C.c_int32(0) for _ in range(4)]
        self._ck(self.lib.fn["read_predict_info"](self.h, C.c_int32(int(slot)), *[C.addressof(x) for x in v]), "read_predict_info")
        return dict(n_listed=int(v[0].value), n_guessed=int(v[1].value), n_ok_guessed=int(v[2].value), fell_back=bool(v[3].value))

    def set_tracker(self, max_cnt=DEFAULT_MAX_CNT, border=DEFAULT_TRACK_BORDER):
        """The reference's MAX_CNT (at most MAX_TRACK_POINTS) and inBorder's margin."""
        self._ck(self.lib.fn["set_tracker"](self.h, C.c_int32(int(max_cnt)), C.c_int32(int(border))), "set_tracker")

    def read_batch(self, imgs, times, slots=None, publish=True):
        """FeatureTracker.read_image followed by update_ids for one new image of each slot, in one call (include/vio_frame_read.h).
        imgs: (height, width) uint8 arrays; times: one time stamp per image, or one for all; slots: default 0 .. len(imgs) - 1.  A list
        of dicts: pts (n, 2) float32, ids (n,) int64 (after updateID), track_cnt (n,) int32, un_pts, velocity (n, 2) float32, and the
        counts n, n_new, n_tracked_in, n_after_track, n_after_reject, reject_status, reject_hyp, n_candidates; status (OK, or NOT_FINITE for
        a slot whose camera could not lift a point: its un_pts and velocity are NaN, or its tracked points were dropped; the call does not
        raise for it) with n_clamped and n_bad of read_lift_info."""
        B = len(imgs)
        slots = list(range(B)) if slots is None else [int(s) for s in slots]
        times = [float(times)] * B if np.isscalar(times) else [float(t) for t in times]
        if len(slots) != B or len(times) != B:
            raise ValueError("one slot and one time per image")
        arr = (VioFrameReadItem * max(B, 1))()
        res = (VioFrameReadResult * max(B, 1))()
        keep, outs = [], []
        R = MAX_TRACK_POINTS
        for i in range(B):
            a = _image(imgs[i])
            o = (np.zeros((R, 2), np.float32), np.zeros(R, np.int64), np.zeros(R, np.int32), np.zeros((R, 2), np.float32), np.zeros((R, 2), np.float32))
            keep.append(a)
            outs.append(o)
            arr[i] = VioFrameReadItem(slots[i], a.shape[1], a.shape[0], a.strides[0], a.ctypes.data, times[i], *[x.ctypes.data for x in o])
        self._ck(self.lib.fn["read_batch"](self.h, C.c_int32(B), C.addressof(arr), C.c_int32(1 if publish else 0), C.addressof(res)), "read_batch",
                 allow_not_finite=True)
        out = []
        for i in range(B):
            self.shapes[slots[i]] = keep[i].shape
            r, n = res[i], int(res[i].n)
            d = dict(zip(("pts", "ids", "track_cnt", "un_pts", "velocity"), (x[:n].copy() for x in outs[i])))
            d.update({k: int(getattr(r, k)) for k in ("status", "n", "n_new", "n_tracked_in", "n_after_track", "n_after_reject", "reject_status",
                                                     "reject_hyp", "n_candidates")})
            d.update(self.read_lift_info(slots[i]))
            out.append(d)
        return out

    def points_set(self, pts, ids=None, track_cnt=None, slot=0):
        """Seeds the slot's points (they lie in its next frame): pts (n, 2); ids default -1, track_cnt default 1."""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        i = np.full(len(p), -1, np.int64) if ids is None else np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        c = np.ones(len(p), np.int32) if track_cnt is None else np.ascontiguousarray(track_cnt, dtype=np.int32).reshape(-1)
        if len(i) != len(p) or len(c) != len(p):
            raise ValueError("ids and track_cnt need one entry per point")
        self._ck(self.lib.fn["points_set"](self.h, C.c_int32(slot), C.c_int32(len(p)), p.ctypes.data, i.ctypes.data, c.ctypes.data), "points_set")

    def points_get(self, slot=0):
        """The slot's resident points: dict(pts, ids, track_cnt, prev_un_ids, prev_un_pts, next_id)."""
        R = MAX_TRACK_POINTS
        n, m, nid = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        p, i, c = np.zeros((R, 2), np.float32), np.zeros(R, np.int64), np.zeros(R, np.int32)
        pi, pp = np.zeros(R, np.int64), np.zeros((R, 2), np.float32)
        self._ck(self.lib.fn["points_get"](self.h, C.c_int32(slot), C.addressof(n), p.ctypes.data, i.ctypes.data, c.ctypes.data, C.addressof(m),
                                           pi.ctypes.data, pp.ctypes.data, C.addressof(nid)), "points_get")
        return dict(pts=p[:n.value].copy(), ids=i[:n.value].copy(), track_cnt=c[:n.value].copy(), prev_un_ids=pi[:m.value].copy(),
                    prev_un_pts=pp[:m.value].copy(), next_id=int(nid.value))

    def read_timing(self):
        """ms of the last read_batch by stage (include/vio_frame_read.h)."""
        t = (C.c_double * 8)()
        self._ck(self.lib.fn["read_timing"](self.h, t), "read_timing")
        return dict(zip(("host_ms", "push_ms", "track_ms", "reject_ms", "detect_ms", "finish_ms", "readback_ms", "total_ms"), t))

    # ---- accounting -----------------------------------------------------------------------
    def counters(self):
        """Bytes moved since creation (include/vio_frame.h)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.lib.fn["counters"](self.h, c), "counters")
        return {"image_up": int(c[0]), "image_down": int(c[1]), "other_up": int(c[2]), "other_down": int(c[3])}

    def timing(self):
        """ms of the last push, track and detect (include/vio_frame.h); waits for the last push."""
        t = (C.c_double * 8)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"push_host_ms": t[0], "push_upload_ms": t[1], "push_clahe_ms": t[2], "push_pyramid_ms": t[3], "track_ms": t[4],
                "track_total_ms": t[5], "detect_ms": t[6], "detect_total_ms": t[7]}
