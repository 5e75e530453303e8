"""frontend.FeatureTracker with `frames` (a frame.FrameHandle's place) over a stand-in composed from the numpy restatements of the
equaliser, the tracker and the detector, on the fixture frames: every array it gives equals what the same three restatements give
when they are passed as equalizer / tracker / detector.  This pins the wiring (what is pushed, which slot, what is tracked from where,
what the detector sees, the mask, min_dist) without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_reference as cr  # noqa: E402
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402
from test_frontend_equalize import CachedEqualizer  # noqa: E402
from test_frontend_reference import MAX_CNT, MIN_DIST, Tracker, check_frames, fixture_frames  # noqa: E402


class StandInFrames:
    """Slots of (prev, next) equalised images, rolled by push, with FrameHandle's method signatures."""

    def __init__(self):
        self.eq, self.tr, self.de = CachedEqualizer(), Tracker(), dr.Detector()
        self.slots, self.masks, self.pushed, self.calls, self.detect_cfg = {}, {}, [], [], None

    def set_config(self, equalize=None, clahe=None, flow=None, detect=None):
        self.detect_cfg = detect
        if detect is not None:
            self.de.set_config(**detect)

    def set_mask(self, mask, slot=0):
        self.masks[slot] = mask

    def push(self, img, slot=0):
        self.pushed.append((slot, img))
        self.slots[slot] = (self.slots.get(slot, (None, None))[1], self.eq.apply(img))

    def track(self, prev_pts, guess=None, slot=0):
        prev, nxt = self.slots[slot]
        assert prev is not None, "tracking needs two frames"
        self.calls.append(("track", slot, len(prev_pts)))
        return self.tr.track(prev, nxt, prev_pts, guess)

    def detect(self, tracked=None, track_cnt=None, max_total=150, slot=0):
        self.calls.append(("detect", slot, 0 if tracked is None else len(tracked)))
        return self.de.detect(self.slots[slot][1], tracked=tracked, track_cnt=track_cnt, mask=self.masks.get(slot), max_total=max_total)


class StandInSequenceFrames(StandInFrames):
    """StandInFrames with the rest of FrameHandle's methods and settings (push_batch, reset, download, track_batch, detect_batch;
    equalize, the CLAHE settings, levels), for tests/frame_sequences.py: the roll, the reset and the change of levels in a few lines."""

    def __init__(self):
        StandInFrames.__init__(self)
        self.levels, self.equalize, self.clahe, self.flow, self.detect_kw = 4, False, {}, {}, {}

    def set_config(self, equalize=None, clahe=None, flow=None, detect=None):
        if equalize is not None:
            self.equalize = bool(equalize)
        if clahe is not None:
            self.clahe = dict(clahe)
        if detect is not None:
            self.detect_kw = dict(detect)
        if flow is not None:
            if flow.get("levels", 4) != self.levels:
                self.slots = {}                              # (the masks stay)
            self.flow, self.levels = dict(flow), flow.get("levels", 4)

    def set_mask(self, mask, slot=0):
        self.masks.pop(slot, None)
        if mask is not None:
            self.masks[slot] = np.ascontiguousarray(mask)

    def push_batch(self, items):
        for it in items:
            img = np.ascontiguousarray(it["img"])
            slot = it.get("slot", 0)
            self.slots[slot] = (self.slots.get(slot, (None, None))[1], cr.apply(img, **self.clahe) if self.equalize else img)

    def push(self, img, slot=0):
        self.push_batch([dict(slot=slot, img=img)])

    def reset(self, slot=0):
        self.slots.pop(slot, None)

    def download(self, slot=0, which=1, level=0):
        assert self.slots[slot][which] is not None and 0 <= level < self.levels
        return fr.pyramid(self.slots[slot][which], self.levels)[level]

    def track_batch(self, items):
        out = []
        for it in items:
            prev, nxt = self.slots[it["slot"]]
            assert prev is not None, "tracking needs two frames"
            res = fr.multi_level(prev, nxt, it["prev_pts"], it.get("guess"), order="wave64", **self.flow)
            out.append(dict(zip(("next_pts", "status", "iterations", "cost"), res)))
        return out

    def detect_batch(self, items):
        return [dr.detect(self.slots[it["slot"]][1], it.get("tracked"), it.get("track_cnt"), self.masks.get(it["slot"]), it["max_total"],
                          **self.detect_kw) for it in items]

    def track(self, prev_pts, guess=None, slot=0):
        return self.track_batch([dict(slot=slot, prev_pts=prev_pts, guess=guess)])[0]

    def detect(self, tracked=None, track_cnt=None, max_total=150, slot=0):
        return self.detect_batch([dict(slot=slot, tracked=tracked, track_cnt=track_cnt, max_total=max_total)])[0]


@pytest.fixture(scope="module")
def handles_run(vio):
    """The three restatements passed as equalizer / tracker / detector."""
    ft = vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST, equalizer=CachedEqualizer())
    return check_frames(ft, fixture_frames())


def test_frames_sequence_equals_the_three_handles(vio, handles_run):
    frames, st = fixture_frames(), StandInFrames()
    ft = vio.FeatureTracker(None, None, max_cnt=MAX_CNT, min_dist=MIN_DIST, frames=st, slot=3)
    outs = check_frames(ft, frames)
    assert len(outs) == len(handles_run) == 3
    for t, (o, r) in enumerate(zip(outs, handles_run)):
        assert o["n_new"] == r["n_new"], t
        for k in ("pts", "ids", "track_cnt"):
            assert o[k].dtype == r[k].dtype and o[k].tobytes() == r[k].tobytes(), (t, k)
    # the raw frames were pushed, once each, into the slot; nothing else was touched
    assert [s for s, _ in st.pushed] == [3, 3, 3] and all(p is f for (_, p), f in zip(st.pushed, frames))
    assert [c[:2] for c in st.calls] == [("detect", 3), ("track", 3), ("detect", 3), ("track", 3), ("detect", 3)]
    assert st.detect_cfg == dict(min_distance=MIN_DIST)
    assert ft.prev_img is None and ft.cur_img is None and ft.tracker is None and ft.detector is None and ft.equalizer is None
    assert ft.n_id == sum(o["n_new"] for o in outs)


def test_mask_goes_to_the_slot(vio):
    mask = np.full(fixture_frames()[0].shape, 255, dtype=np.uint8)
    st = StandInFrames()
    vio.FeatureTracker(None, None, mask=mask, frames=st, slot=2)
    assert list(st.masks) == [2] and st.masks[2] is mask
    st = StandInFrames()
    vio.FeatureTracker(None, None, frames=st)
    assert st.masks == {}


def test_bad_image_is_refused_before_the_push(vio):
    st = StandInFrames()
    ft = vio.FeatureTracker(None, None, frames=st)
    with pytest.raises(ValueError):
        ft.read_image(np.zeros((4, 4), dtype=np.float32), 0.0)
    assert st.pushed == []
