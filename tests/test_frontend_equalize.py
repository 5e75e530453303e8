"""frontend.FeatureTracker with an equalizer (the reference's EQUALIZE, feature_tracker.cpp:87-95) over the numpy restatements of the
equaliser, the tracker and the detector on the fixture frames: check_frames' invariants hold, the tracker and the detector are handed
the equalised images and nothing else, and without an equalizer the front end does what it did before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_reference as cr  # noqa: E402
import detect_reference as dr  # noqa: E402
from test_frontend_reference import MAX_CNT, MIN_DIST, Tracker, check_frames, fixture_frames  # noqa: E402

_cache = {}


def equalised_frames():
    if "eq" not in _cache:
        _cache["eq"] = [cr.apply(f) for f in fixture_frames()[:2]]
    a, b = _cache["eq"]
    return [a, b, a]


class CachedEqualizer:
    """The restatement, computed once per distinct fixture frame."""

    def __init__(self):
        self.seen = []

    def apply(self, img):
        self.seen.append(img)
        frames = fixture_frames()
        for k in range(2):
            if img.tobytes() == frames[k].tobytes():
                return equalised_frames()[k]
        return cr.apply(img)


class SpyTracker(Tracker):
    def __init__(self):
        self.seen = []

    def track(self, img_prev, img_next, pts, guess=None):
        self.seen.append((img_prev, img_next))
        return Tracker.track(self, img_prev, img_next, pts, guess)


class SpyDetector(dr.Detector):
    def __init__(self):
        dr.Detector.__init__(self)
        self.seen = []

    def detect(self, img, *a, **kw):
        self.seen.append(img)
        return dr.Detector.detect(self, img, *a, **kw)


def run(vio, equalizer, frames):
    tr, de = SpyTracker(), SpyDetector()
    ft = vio.FeatureTracker(tr, de, max_cnt=MAX_CNT, min_dist=MIN_DIST, equalizer=equalizer)
    outs = check_frames(ft, frames)
    return ft, tr, de, outs


@pytest.fixture(scope="module")
def plain(vio):
    """The front end without an equalizer on the equalised frames: what the one with an equalizer must do on the raw ones."""
    return run(vio, None, equalised_frames())


def test_equalised_sequence(vio, plain):
    frames, eq_frames = fixture_frames(), equalised_frames()
    eq = CachedEqualizer()
    ft, tr, de, outs = run(vio, eq, frames)
    # the equaliser saw the raw frames, the tracker and the detector the equalised ones
    assert len(eq.seen) == 3 and all(s.tobytes() == f.tobytes() for s, f in zip(eq.seen, frames))
    assert len(de.seen) == 3 and all(s.tobytes() == f.tobytes() for s, f in zip(de.seen, eq_frames))
    assert len(tr.seen) == 2
    assert tr.seen[0][0].tobytes() == eq_frames[0].tobytes() and tr.seen[0][1].tobytes() == eq_frames[1].tobytes()
    assert tr.seen[1][0].tobytes() == eq_frames[1].tobytes() and tr.seen[1][1].tobytes() == eq_frames[2].tobytes()
    assert ft.cur_img.tobytes() == eq_frames[2].tobytes() and ft.prev_img.tobytes() == eq_frames[1].tobytes()
    # the first frame's corners are the detector's on the equalised image, and they differ from those of the raw one
    first = dr.detect(eq_frames[0])
    assert outs[0]["n_new"] == first["n_new"] and np.array_equal(outs[0]["pts"], first["new_pts"])
    raw_first = dr.detect(frames[0])
    assert not (raw_first["n_new"] == first["n_new"] and np.array_equal(raw_first["new_pts"], first["new_pts"]))
    # equalising inside the front end is equalising before it
    _, _, _, ref = plain
    for o, r in zip(outs, ref):
        assert o["n_new"] == r["n_new"]
        for k in ("pts", "ids", "track_cnt"):
            assert o[k].tobytes() == r[k].tobytes(), k
    assert ft.n_id == sum(o["n_new"] for o in outs)


def test_no_equalizer_is_what_it_was(vio):
    frames = fixture_frames()
    ft, tr, de, outs = run(vio, None, frames)
    assert ft.equalizer is None
    assert all(s is f for s, f in zip(de.seen, frames))           # the very arrays: nothing touched the images
    old = vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST)     # (the call as it was: no equalizer argument)
    ref = check_frames(old, frames)
    for o, r in zip(outs, ref):
        for k in ("pts", "ids", "track_cnt"):
            assert o[k].tobytes() == r[k].tobytes(), k
    first = dr.detect(frames[0])
    assert np.array_equal(outs[0]["pts"], first["new_pts"])


def test_equalizer_result_is_checked(vio):
    class Bad:
        def apply(self, img):
            return img.astype(np.float32)

    ft = vio.FeatureTracker(Tracker(), dr.Detector(), equalizer=Bad())
    with pytest.raises(ValueError):
        ft.read_image(fixture_frames()[0], 0.0)
