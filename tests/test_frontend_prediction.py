"""FeatureTracker.set_prediction and the prediction= fallback with stub trackers and no device: the guess array is the predicted pixel
for a current point whose id is listed and the point's own pixel for every other, it is used for one frame, without a prediction the
tracker is called without a guess keyword, and the fallback tracks a second time exactly when fewer than min_tracked statuses are 0.
The same through frames=."""
import numpy as np
import pytest

SHAPE = (60, 80)


class StubDetector:
    """Keeps every tracked point and adds `new` fixed points on the first call."""

    def __init__(self, new):
        self.new, self.calls = np.asarray(new, dtype=np.float32), 0

    def detect(self, img, tracked=None, track_cnt=None, mask=None, max_total=150):
        self.calls += 1
        n = 0 if tracked is None else len(tracked)
        return dict(keep_order=np.arange(n), new_pts=self.new if self.calls == 1 else np.zeros((0, 2), dtype=np.float32))


class StrictTracker:
    """A tracker whose track has no guess parameter at all, as the stubs of the older tests: a guess keyword would be a TypeError."""

    def __init__(self):
        self.calls = []

    def track(self, img_prev, img_next, pts):
        self.calls.append(np.array(pts))
        return dict(next_pts=np.asarray(pts, dtype=np.float32) + 1.0, status=np.zeros(len(pts), dtype=np.int32))


class GuessTracker:
    """Records every call's keywords; moves every point by +1; `lost(call, n)` gives the statuses."""

    def __init__(self, lost=None):
        self.calls, self.lost = [], lost

    def track(self, img_prev, img_next, pts, **kw):
        self.calls.append(dict(pts=np.array(pts), kw={k: (None if v is None else np.array(v)) for k, v in kw.items()}))
        st = np.zeros(len(pts), dtype=np.int32) if self.lost is None else np.asarray(self.lost(len(self.calls), len(pts)), dtype=np.int32)
        return dict(next_pts=np.asarray(pts, dtype=np.float32) + 1.0, status=st)


class StubFrames:
    """frames=: push, track(prev_pts, slot=, [guess=]) and detect of FrameHandle's signatures."""

    def __init__(self, new):
        self.calls, self.det = [], StubDetector(new)

    def push(self, img, slot=0):
        pass

    def track(self, prev_pts, slot=0, **kw):
        self.calls.append(dict(pts=np.array(prev_pts), slot=slot, kw={k: np.array(v) for k, v in kw.items()}))
        return dict(next_pts=np.asarray(prev_pts, dtype=np.float32) + 1.0, status=np.zeros(len(prev_pts), dtype=np.int32))

    def detect(self, tracked=None, track_cnt=None, max_total=150, slot=0):
        return self.det.detect(None, tracked=tracked, track_cnt=track_cnt, max_total=max_total)


NEW = np.array([[10, 10], [20, 12], [30, 14], [40, 16], [50, 18], [60, 20]], dtype=np.float32)
IMG = np.zeros(SHAPE, dtype=np.uint8)


def started(vio, tracker, **kw):
    ft = vio.FeatureTracker(tracker, StubDetector(NEW), border=1, **kw)
    ft.read_image(IMG, 0.0)
    ft.update_ids()                                         # ids 0 .. 5 at NEW
    return ft


def test_without_a_prediction_the_tracker_gets_no_guess_keyword(vio):
    tr = StrictTracker()
    ft = started(vio, tr)
    ft.read_image(IMG, 1.0)
    ft.read_image(IMG, 2.0)
    assert len(tr.calls) == 2 and np.array_equal(tr.calls[0], NEW) and np.array_equal(tr.calls[1], NEW + 1.0)
    assert ft.pred_info == dict(n_guessed=0, fell_back=False)
    g = GuessTracker()
    ft = started(vio, g, prediction=dict(min_tracked=3))    # the fallback alone does not add the keyword either
    ft.read_image(IMG, 1.0)
    assert [c["kw"] for c in g.calls] == [{}]


def test_guess_is_composed_by_the_rule_and_used_once(vio):
    tr = GuessTracker()
    ft = started(vio, tr)
    pred_ids = np.array([4, 99, 1, -1, 4], dtype=np.int64)   # 99: no such point; -1: never a point's id here; 4 twice: the first counts
    pred_px = np.array([[41.5, 17.25], [1, 1], [22.5, 11.75], [7, 7], [0, 0]])
    ft.set_prediction(pred_ids, pred_px)
    ft.read_image(IMG, 1.0)
    assert len(tr.calls) == 1 and list(tr.calls[0]["kw"]) == ["guess"]
    want = NEW.copy()
    want[4], want[1] = [41.5, 17.25], [22.5, 11.75]
    g = tr.calls[0]["kw"]["guess"]
    assert g.dtype == np.float32 and g.tobytes() == want.tobytes() and np.array_equal(tr.calls[0]["pts"], NEW)
    assert ft.pred_info == dict(n_guessed=2, fell_back=False)
    ft.read_image(IMG, 2.0)                                 # the frame after: no guess
    assert len(tr.calls) == 2 and tr.calls[1]["kw"] == {}
    assert ft.pred_info == dict(n_guessed=0, fell_back=False)


def test_new_points_never_take_a_prediction(vio):
    tr = GuessTracker()
    ft = vio.FeatureTracker(tr, StubDetector(NEW), border=1)
    ft.read_image(IMG, 0.0)                                 # no update_ids: every id is -1
    ft.set_prediction([-1], [[5.0, 5.0]])
    ft.read_image(IMG, 1.0)
    assert tr.calls[0]["kw"]["guess"].tobytes() == NEW.tobytes() and ft.pred_info["n_guessed"] == 0


def test_a_prediction_set_before_the_first_image_is_dropped(vio):
    tr = GuessTracker()
    ft = vio.FeatureTracker(tr, StubDetector(NEW), border=1)
    ft.set_prediction([0], [[5.0, 5.0]])
    ft.read_image(IMG, 0.0)                                 # no points yet: no call
    ft.update_ids()
    ft.read_image(IMG, 1.0)
    assert len(tr.calls) == 1 and tr.calls[0]["kw"] == {}


@pytest.mark.parametrize("n_ok,min_tracked,again", [(6, 6, False), (5, 6, True), (0, 1, True), (0, 0, False), (3, 3, False), (2, 3, True)])
def test_fallback_tracks_again_exactly_below_min_tracked(vio, n_ok, min_tracked, again):
    lost = lambda call, n: [0] * n if call > 1 else [0] * n_ok + [1] * (n - n_ok)      # the guessed call loses n - n_ok points
    tr = GuessTracker(lost)
    ft = started(vio, tr, prediction=dict(min_tracked=min_tracked))
    ft.set_prediction([0, 1, 2], NEW[:3] + 0.5)
    out = ft.read_image(IMG, 1.0)
    assert len(tr.calls) == (2 if again else 1)
    assert list(tr.calls[0]["kw"]) == ["guess"]
    if again:
        assert tr.calls[1]["kw"] == {} and np.array_equal(tr.calls[1]["pts"], NEW) and len(out["ids"]) == 6
    else:
        assert len(out["ids"]) == n_ok
    assert ft.pred_info == dict(n_guessed=3, fell_back=again)


def test_no_fallback_by_default(vio):
    tr = GuessTracker(lambda call, n: [1] * n)
    ft = started(vio, tr)
    ft.set_prediction([0], NEW[:1])
    out = ft.read_image(IMG, 1.0)
    assert len(tr.calls) == 1 and len(out["ids"]) == 0


def test_through_frames(vio):
    fr = StubFrames(NEW)
    ft = vio.FeatureTracker(None, None, frames=fr, slot=3, border=1)
    ft.read_image(IMG, 0.0)
    ft.update_ids()
    ft.read_image(IMG, 1.0)
    assert fr.calls[0]["kw"] == {} and fr.calls[0]["slot"] == 3
    ft.set_prediction([2, 5], [[31.5, 15.5], [61.0, 21.0]])
    ft.read_image(IMG, 2.0)
    want = NEW + 1.0
    want[2], want[5] = [31.5, 15.5], [61.0, 21.0]
    assert list(fr.calls[1]["kw"]) == ["guess"] and fr.calls[1]["kw"]["guess"].tobytes() == want.astype(np.float32).tobytes()
    assert fr.calls[1]["slot"] == 3
    ft.read_image(IMG, 3.0)
    assert fr.calls[2]["kw"] == {}


def test_set_prediction_checks_its_arguments(vio):
    ft = vio.FeatureTracker(GuessTracker(), StubDetector(NEW))
    with pytest.raises(ValueError, match="same length"):
        ft.set_prediction([1, 2], [[0.0, 0.0]])
