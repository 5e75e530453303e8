"""FeatureTracker: an image sequence in, ids with tracks out.  It composes the tracker (flow.FlowHandle) and the detector
(detect.DetectHandle) the way FeatureTracker::readImage (VM/src/feature_tracker.cpp:97-164) and updateID (:204-214) do:

    ft = FeatureTracker(vio.load_flow().create(), vio.load_detect().create())
    for t, img in frames:
        out = ft.read_image(img, t)            # dict(pts (n, 2) float32, ids (n,), track_cnt (n,)); ids are -1 for new points ...
        ft.update_ids()                        # ... until this gives them the next free ids
        ids, rows = ft.feature_frame()         # (with a rejecter) what the reference publishes to the estimator

read_image tracks cur_pts into the new image, drops the points the tracker lost and those whose rounded position is outside `border`,
adds one to every track_cnt, and on a published frame runs `reject` (if given), then setMask and the detection (which keeps at most
max_cnt points min_dist apart, the long tracks first), then addPoints (id -1, count 1); last it rolls prev / cur.

`tracker` and `detector` are any objects with .track(img_prev, img_next, pts) -> dict(next_pts, status) and
.detect(img, tracked=, track_cnt=, mask=, max_total=) -> dict(keep_order, new_pts) of the handles' signatures; a detector with a
set_config gets min_distance = min_dist (its other settings return to their defaults).  reject(cur_pts, forw_pts) -> a boolean array,
True for the pairs to keep: the place of rejectWithF.

`rejecter` is a reject.RejectHandle with its camera set, or any object with .reject(cur, forw, pair) -> a boolean array and
.undistort(pts, ids, prev_ids, prev_un_pts, dt) -> (un_pts, velocity).  With one, read_image runs rejectWithF (feature_tracker.cpp:169-202)
where the hook stands, with pair = the count of frames read, and after rolling prev / cur it runs undistortedPoints (:258-306): the
dict gains un_pts (n, 2) float32, the normalised points, and velocity (n, 2) float32.  The previous frame's ids are kept as they were
when its points were undistorted, before update_ids: a new point still carried -1 then, so its velocity is zero in its first two frames,
as in the reference.  feature_frame() returns what the reference publishes.  With rejecter=None nothing of this happens.

`equalizer` is a clahe.ClaheHandle, or any object with .apply(img) -> a uint8 image of the same shape: the reference's EQUALIZE
(feature_tracker.cpp:87-95).  With one, read_image equalises the image first, so the tracker, the detector and cur_img / prev_img see
equalised images only, as in the reference.  With equalizer=None nothing of this happens.

`frames` is a frame.FrameHandle, or any object with .push(img, slot=), .track(prev_pts, slot=) and .detect(tracked=, track_cnt=,
max_total=, slot=) of the handle's signatures (and .set_mask(mask, slot=) if a mask is given, .set_config(detect=) if it has one).  With
one, read_image pushes the raw image into `slot` and tracks and detects through it: the image is uploaded once, and equalising is the
handle's business (its equalize setting), so tracker, detector and equalizer may be None and are not used.  prev_img / cur_img stay
None; frames.download(slot, PREV or NEXT) gives them.  With frames=None nothing of this happens.

The camera models besides PINHOLE (KANNALA_BRANDT for FISHEYE, MEI, SCARAMUZZA): pass a camera.CameraHandle (or its bind(slot) view) as
`rejecter`; it has RejectHandle's .reject / .undistort.  On the resident read_batch path (BatchFeatureTracker) every slot may have a camera
of its own, of any of the four models: cameras={slot: dict(model=, width=, height=, ...)} (frame.FrameHandle.set_slot_camera).  Missing
against the reference: the fisheye circle mask as a built-in (it is the `mask` image).
BatchFeatureTracker is the same front end for many streams at once over a frame.FrameHandle's read_batch: the points stay on the
device, one call reads one new image of every stream.

`flow_back` is None, or a dict of FlowHandle.set_back's arguments (levels, max_dist): the forward-backward check of VINS-Fusion's front
end (include/vio_flow_back.h), set on `frames` if given and else on `tracker`.  A point that fails it has a status other than 0, so it
leaves with those the tracker lost; back_info holds the check's counts of the last read_image.  reject_with_f=False skips
rejecter.reject on a published frame, as VINS-Fusion does, and keeps rejecter.undistort.  BatchFeatureTracker takes the same two.  With
both left at their defaults the classes make exactly the calls they made without them.

Prediction (VINS-Fusion's predictPtsInNextFrame / setPrediction): predict_pixels(fm, camera, ...) gives the pixels
the tracks with a depth are expected at in the next image, set_prediction(ids, pixels) hands them to the next read_image, which passes
guess= to the tracker (FlowHandle.track, or FrameHandle.track with frames=): the predicted pixel for a current point whose id is
listed, the point's current pixel for every other.  A prediction is used for one frame.  prediction=dict(min_tracked=10) is
VINS-Fusion's fallback: fewer than min_tracked points with status 0 from the guessed call, and the frame is tracked again without a
guess.  pred_info holds n_guessed and fell_back of the last read_image.  Without a prediction the tracker is called as before, with no
guess keyword.  BatchFeatureTracker takes the same: set_predictions({slot: (ids, pixels)}) hands them to the next read_images
(frame.FrameHandle.set_prediction_batch, include/vio_frame_predict.h), the ids are joined and the fallback is decided on the device, and
every array still equals the per-stream loop's.  predict_pixels_batch is predict_pixels for many slots in two library calls.

One thing differs on purpose: prev_pts stays aligned with the points through setMask's
reordering (the reference reorders forw_pts, ids and track_cnt and leaves prev_pts as it was).
"""
import numpy as np

from .flow import FAIL_BACK_FAR, FAIL_BACK_LOST


class FeatureTracker:
    def __init__(self, tracker, detector, max_cnt=150, min_dist=30, border=1, reject=None, mask=None, rejecter=None, equalizer=None, frames=None,
                 slot=0, flow_back=None, reject_with_f=True, prediction=None):
        self.tracker, self.detector = tracker, detector
        self.min_tracked = None if prediction is None else int(dict(prediction).get("min_tracked", 0))
        self.pred_ids, self.pred_pts = None, None          # set_prediction's, until the next read_image
        self.pred_info = dict(n_guessed=0, fell_back=False)
        self.frames, self.slot = frames, int(slot)
        self.flow_back, self.reject_with_f = flow_back, bool(reject_with_f)
        self.back_info = dict(n_checked=0, n_back_lost=0, n_back_far=0)
        if flow_back is not None:
            if frames is not None:
                frames.set_flow_back(**dict(flow_back))
            else:
                tracker.set_back(**dict(flow_back))
        self.max_cnt, self.min_dist, self.border, self.reject, self.mask = int(max_cnt), int(min_dist), int(border), reject, mask
        if frames is not None:
            if hasattr(frames, "set_config"):
                frames.set_config(detect=dict(min_distance=self.min_dist))
            if mask is not None:
                frames.set_mask(mask, slot=self.slot)
        elif hasattr(detector, "set_config"):
            detector.set_config(min_distance=self.min_dist)
        self.prev_img = self.cur_img = None
        self.prev_pts = np.zeros((0, 2), dtype=np.float32)
        self.cur_pts = np.zeros((0, 2), dtype=np.float32)
        self.ids = np.zeros(0, dtype=np.int64)
        self.track_cnt = np.zeros(0, dtype=np.int32)
        self.n_new = 0                          # the points the last read_image added
        self.n_id = 0
        self.cur_time = self.prev_time = None
        self.rejecter = rejecter
        self.equalizer = equalizer
        self.n_frames = 0                       # the frames read: rejectWithF's `pair`
        self.cur_un_pts = np.zeros((0, 2), dtype=np.float32)
        self.velocity = np.zeros((0, 2), dtype=np.float32)
        self.prev_un_ids = np.zeros(0, dtype=np.int64)         # prev_un_pts_map: the ids and the normalised points of the frame before
        self.prev_un_pts = np.zeros((0, 2), dtype=np.float32)

    def in_border(self, pts, shape):
        """readImage's inBorder on the rounded positions (cvRound: ties to even) in an image of `shape`."""
        h, w = shape
        with np.errstate(invalid="ignore"):
            r = np.rint(np.asarray(pts, dtype=np.float64).reshape(-1, 2))
        b = self.border
        return (b <= r[:, 0]) & (r[:, 0] < w - b) & (b <= r[:, 1]) & (r[:, 1] < h - b)

    def _reduce(self, keep, *arrays):
        return [a[keep] for a in arrays]

    def set_prediction(self, ids, pixels):
        """VINS-Fusion's setPrediction: the pixels (n, 2) the tracks `ids` (n,) are expected at in the next image (predict_pixels).  The
        next read_image starts the Lucas-Kanade search of a current point whose id is listed from its predicted pixel and of every
        other point from its current pixel; the prediction is used for that one frame and then dropped."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        pix = np.asarray(pixels, dtype=np.float32).reshape(-1, 2)
        if len(ids) != len(pix):
            raise ValueError("ids and pixels must have the same length")
        self.pred_ids, self.pred_pts = ids.copy(), pix.copy()

    def _take_guess(self, cur, ids):
        """The guess array of the frame from the prediction (None without one), which is dropped."""
        pred_ids, pred_pts = self.pred_ids, self.pred_pts
        self.pred_ids = self.pred_pts = None
        self.pred_info = dict(n_guessed=0, fell_back=False)
        if pred_ids is None:
            return None
        guess = np.array(cur, dtype=np.float32).reshape(-1, 2)
        order = np.argsort(pred_ids, kind="stable")
        at = np.searchsorted(pred_ids[order], ids)
        hit = (at < len(order)) & (ids >= 0)
        hit[hit] = pred_ids[order][at[hit]] == ids[hit]
        guess[hit] = pred_pts[order][at[hit]]
        self.pred_info["n_guessed"] = int(np.sum(hit))
        return guess

    def _track(self, img, cur, guess):
        """One call of the tracker; without a guess exactly the call made before there were predictions."""
        if guess is None:
            return self.frames.track(cur, slot=self.slot) if self.frames is not None else self.tracker.track(self.cur_img, img, cur)
        if self.frames is not None:
            return self.frames.track(cur, guess=guess, slot=self.slot)
        return self.tracker.track(self.cur_img, img, cur, guess=guess)

    def read_image(self, img, t, publish=True):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("an image must be a 2-d uint8 array")
        if self.frames is not None:
            self.frames.push(img, slot=self.slot)
        elif self.equalizer is not None:
            img = np.asarray(self.equalizer.apply(img))
            if img.dtype != np.uint8 or img.ndim != 2:
                raise ValueError("the equalizer must return a 2-d uint8 array")
        self.prev_time, self.cur_time = self.cur_time, t
        if self.frames is None and self.cur_img is None:
            self.prev_img = self.cur_img = img
        cur, forw = self.cur_pts, np.zeros((0, 2), dtype=np.float32)
        ids, cnt = self.ids, self.track_cnt
        if self.flow_back is not None:
            self.back_info = dict(n_checked=0, n_back_lost=0, n_back_far=0)
        guess = self._take_guess(cur, ids)
        if len(cur) > 0:
            out = self._track(img, cur, guess)
            if guess is not None and self.min_tracked is not None and int(np.sum(np.asarray(out["status"]) == 0)) < self.min_tracked:
                out = self._track(img, cur, None)           # VINS-Fusion's fallback: the frame again from the old pixels
                self.pred_info["fell_back"] = True
            forw =np.asarray(out["next_pts"], dtype=np.float32).reshape(-1, 2)
            if self.flow_back is not None:
                st = np.asarray(out["status"])
                self.back_info = dict(n_checked=int(np.sum((st == 0) | (st == FAIL_BACK_LOST) | (st == FAIL_BACK_FAR))),
                                      n_back_lost=int(np.sum(st == FAIL_BACK_LOST)), n_back_far=int(np.sum(st == FAIL_BACK_FAR)))
            ok = (np.asarray(out["status"]) == 0) & self.in_border(forw, img.shape)
            cur, forw, ids, cnt = self._reduce(ok, cur, forw, ids, cnt)
        cnt = cnt + 1
        self.n_new = 0
        if publish:
            if self.reject is not None and len(forw) > 0:
                ok = np.asarray(self.reject(cur, forw), dtype=bool).reshape(-1)
                cur, forw, ids, cnt = self._reduce(ok, cur, forw, ids, cnt)
            if self.rejecter is not None and self.reject_with_f and len(forw) > 0:
                ok = np.asarray(self.rejecter.reject(cur, forw, self.n_frames), dtype=bool).reshape(-1)
                cur, forw, ids, cnt = self._reduce(ok, cur, forw, ids, cnt)
            if self.frames is not None:
                det = self.frames.detect(tracked=forw, track_cnt=cnt, max_total=self.max_cnt, slot=self.slot)
            else:
                det = self.detector.detect(img, tracked=forw, track_cnt=cnt, mask=self.mask, max_total=self.max_cnt)
            order = np.asarray(det["keep_order"], dtype=np.int64)
            new = np.asarray(det["new_pts"], dtype=np.float32).reshape(-1, 2)
            self.n_new = len(new)
            cur = np.concatenate([cur[order], np.full((len(new), 2), np.nan, dtype=np.float32)])
            forw = np.concatenate([forw[order], new])
            ids = np.concatenate([ids[order], np.full(len(new), -1, dtype=np.int64)])
            cnt = np.concatenate([cnt[order], np.ones(len(new), dtype=np.int32)]).astype(np.int32)
        if self.frames is None:
            self.prev_img, self.cur_img = self.cur_img, img
        self.prev_pts, self.cur_pts = cur, forw
        self.ids, self.track_cnt = ids, cnt
        self.n_frames += 1
        out = dict(pts=self.cur_pts.copy(), ids=self.ids.copy(), track_cnt=self.track_cnt.copy())
        if self.rejecter is not None:
            dt = None if self.prev_time is None else self.cur_time - self.prev_time
            un, vel = self.rejecter.undistort(self.cur_pts, self.ids, self.prev_un_ids, self.prev_un_pts, dt)
            self.cur_un_pts = np.asarray(un, dtype=np.float32).reshape(-1, 2)
            self.velocity = np.asarray(vel, dtype=np.float32).reshape(-1, 2)
            self.prev_un_ids, self.prev_un_pts = self.ids.copy(), self.cur_un_pts.copy()       # (before update_ids: the quirk above)
            out.update(un_pts=self.cur_un_pts.copy(), velocity=self.velocity.copy())
        return out

    def feature_frame(self):
        """What the reference publishes of the frame (System::PubImageData, VM/src/System.cpp:228-250): the points with track_cnt > 1,
        as (ids (n,) int64, rows (n, 7) float64 of x, y, 1, u, v, vx, vy), the per-frame input of FeatureManager and processImage.  Call
        it after update_ids; it needs a rejecter."""
        if self.rejecter is None:
            raise RuntimeError("feature_frame needs a rejecter: the normalised points and the velocities are its")
        k = np.nonzero(self.track_cnt > 1)[0]
        rows = np.zeros((len(k), 7), dtype=np.float64)
        rows[:, 0:2] = self.cur_un_pts[k]
        rows[:, 2] = 1.0
        rows[:, 3:5] = self.cur_pts[k]
        rows[:, 5:7] = self.velocity[k]
        return self.ids[k].copy(), rows

    def update_ids(self):
        """updateID over every point: a new point (id -1) gets the next free id.  Returns the ids."""
        new = np.nonzero(self.ids == -1)[0]
        self.ids[new] = self.n_id + np.arange(len(new))
        self.n_id += len(new)
        return self.ids.copy()


class BatchFeatureTracker:
    """FeatureTracker(frames=, rejecter=, slot=s) followed by update_ids, for every slot of `slots` in one call per frame: the join of
    the steps runs on the device (frame.FrameHandle.read_batch, include/vio_frame_read.h), the points never leave it, and every array equals
    the per-stream loop's byte for byte.

        bt = BatchFeatureTracker(frames, slots=range(64), max_cnt=150, min_dist=30)       # frames.set_camera(...) first
        outs = bt.read_images(imgs, t)               # dicts of pts, ids (after updateID), track_cnt, un_pts, velocity, n_new
        for ids, rows in bt.feature_frames(): ...    # per slot, FeatureTracker.feature_frame()'s pair

    masks: None, or {slot: mask}.  cameras: None, or {slot: set_slot_camera's keywords}: the slot's own camera, of any model; a slot
    without one lifts through the handle's (frames.set_camera).  The handle's detector gets min_distance = min_dist (its other settings return to their defaults), as
    in FeatureTracker.  flow_back, reject_with_f: FeatureTracker's (frame.FrameHandle.set_flow_back, set_reject_with_f); frames.read_back_info(slot)
    has the check's counts.  prediction: None, or dict(min_tracked=k): FeatureTracker's fallback, armed on the handle
    (frame.FrameHandle.set_prediction_fallback); None leaves the handle as it is.  set_predictions hands predicted pixels to the next
    read_images, and pred_info holds, per slot, n_guessed and fell_back of the last one."""

    def __init__(self, frames, slots, max_cnt=150, min_dist=30, border=1, masks=None, cameras=None, flow_back=None, reject_with_f=True,
                 prediction=None):
        self.frames, self.slots = frames, [int(s) for s in slots]
        if len(set(self.slots)) != len(self.slots):
            raise ValueError("a slot is listed twice")
        self.max_cnt, self.min_dist, self.border = int(max_cnt), int(min_dist), int(border)
        frames.set_config(detect=dict(min_distance=self.min_dist))
        frames.set_tracker(max_cnt=self.max_cnt, border=self.border)
        for s, m in (masks or {}).items():
            frames.set_mask(m, slot=int(s))
        for s, cam in (cameras or {}).items():
            frames.set_slot_camera(int(s), **cam)
        if flow_back is not None:
            frames.set_flow_back(**dict(flow_back))
        if not reject_with_f:
            frames.set_reject_with_f(False)
        if prediction is not None:
            frames.set_prediction_fallback(int(dict(prediction).get("min_tracked", 0)))
        self.predicted = set()                                  # the slots set_predictions named since the last read_images
        self.pred_info = [dict(n_guessed=0, fell_back=False) for _ in self.slots]
        self.last = [None] * len(self.slots)

    def set_predictions(self, predictions):
        """{slot: (ids (n,), pixels (n, 2))}: FeatureTracker.set_prediction for each named slot, in one call.  The next read_images uses
        them and drops them; a slot named again before it takes the later prediction."""
        items = [(int(s), ids, pix) for s, (ids, pix) in dict(predictions).items()]
        unknown = [s for s, _, _ in items if s not in self.slots]
        if unknown:
            raise ValueError("slot %d is not one of this tracker's" % unknown[0])
        if items:
            self.frames.set_prediction_batch(items)
            self.predicted.update(s for s, _, _ in items)

    def read_images(self, imgs, t, publish=True):
        """One new image per slot, in the order of `slots`; t: one time stamp for all, or one per image.  Returns read_batch's dicts."""
        if len(imgs) != len(self.slots):
            raise ValueError("one image per slot")
        for img in imgs:
            a = np.asarray(img)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError("an image must be a 2-d uint8 array")
        self.last = self.frames.read_batch(imgs, t, slots=self.slots, publish=publish)
        predicted, self.predicted = self.predicted, set()       # (the read consumed them)
        self.pred_info = [dict(n_guessed=0, fell_back=False) for _ in self.slots]
        for k, s in enumerate(self.slots):
            if s in predicted:
                info = self.frames.read_predict_info(s)
                self.pred_info[k] = dict(n_guessed=int(info["n_guessed"]), fell_back=bool(info["fell_back"]))
        return self.last

    def feature_frames(self):
        """Per slot what the reference publishes of its last frame: (ids (n,) int64, rows (n, 7) float64 of x, y, 1, u, v, vx, vy) of the
        points with track_cnt > 1."""
        out = []
        for o in self.last:
            if o is None:
                raise RuntimeError("feature_frames needs a frame: call read_images first")
            k = np.nonzero(o["track_cnt"] > 1)[0]
            rows = np.zeros((len(k), 7), dtype=np.float64)
            rows[:, 0:2] = o["un_pts"][k]
            rows[:, 2] = 1.0
            rows[:, 3:5] = o["pts"][k]
            rows[:, 5:7] = o["velocity"][k]
            out.append((o["ids"][k].copy(), rows))
        return out


def predict_pixels_batch(fm, camera, items, width=None, height=None):
    """predict_pixels for many slots in one fm.predict_batch and one camera.project_batch, two library calls whatever len(items) is.
    items: dicts of frame_count, poses, ext and, optionally, next_pose (None), fm_slot (0), camera_slot (None: the camera handle's
    own), width and height (default: this call's).  Returns one (ids, pixels) per item, each what predict_pixels gives for it:
    BatchFeatureTracker.set_predictions takes {slot: pair}."""
    items = [dict(it) for it in items]
    preds = fm.predict_batch([(it.get("fm_slot", 0), it["frame_count"], it["poses"], it["ext"], it.get("next_pose")) for it in items])
    pitems = []
    for it, pred in zip(items, preds):
        item = dict(points=pred["pts_cam"])
        if it.get("camera_slot") is not None:
            item["slot"] = int(it["camera_slot"])
        pitems.append(item)
    projs = camera.project_batch(pitems)
    out = []
    for it, pred, proj in zip(items, preds, projs):
        pix = proj["pixels"]
        ok = proj["flags"] == 0
        w, h = it.get("width", width), it.get("height", height)
        if w is not None and h is not None:
            with np.errstate(invalid="ignore"):
                ok &= (pix[:, 0] >= 0) & (pix[:, 0] <= w - 1) & (pix[:, 1] >= 0) & (pix[:, 1] <= h - 1)
        out.append((pred["ids"][ok].copy(), pix[ok].copy()))
    return out


def predict_pixels(fm, camera, frame_count, poses, ext, next_pose=None, fm_slot=0, camera_slot=None, width=None, height=None):
    """VINS-Fusion's predictPtsInNextFrame and setPrediction's projection composed: the tracks of slot `fm_slot` of the fm.FmHandle
    `fm` that have a depth and end at frame_count, moved into the camera of the next pose (FmHandle.predict_batch; next_pose None: the
    constant-velocity pose) and projected by camera slot `camera_slot` of the camera.CameraHandle `camera` (project_batch).  Returns
    (ids (m,) int64, pixels (m, 2) float64) of the predictions whose flag is 0 and, where width and height are given, whose pixel lies
    inside the image (0 <= u <= width - 1, 0 <= v <= height - 1): FeatureTracker.set_prediction's arguments."""
    return predict_pixels_batch(fm, camera, [dict(frame_count=frame_count, poses=poses, ext=ext, next_pose=next_pose, fm_slot=fm_slot,
                                                  camera_slot=camera_slot)], width=width, height=height)[0]
