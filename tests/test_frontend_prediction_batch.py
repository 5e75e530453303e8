"""frontend.predict_pixels_batch and BatchFeatureTracker.set_predictions / pred_info with stub handles and no device, as
tests/test_frontend_prediction.py does for FeatureTracker: the batch makes two library calls whatever the count of items, each item's
result is predict_pixels' for it, predict_pixels is its one-item case, a prediction reaches the handle in one call and belongs to the
next read_images only, and without one the handle sees exactly the calls it saw before."""
import numpy as np
import pytest


class StubFm:
    """predict_batch of FmHandle's signature: item k of slot s predicts ids 100 s + (0 .. n - 1) at points that depend on s and fc."""

    def __init__(self):
        self.calls = []

    def predict_batch(self, items):
        self.calls.append([(s, fc, nxt is not None) for s, fc, _, _, nxt in items])
        out = []
        for s, fc, poses, ext, nxt in items:
            n = 3 + s
            pts = np.stack([np.arange(n) * 10.0 + s, np.arange(n) * 7.0 - fc, np.full(n, 2.0 if nxt is None else 4.0)], axis=1)
            out.append(dict(ids=100 * s + np.arange(n, dtype=np.int64), pts_cam=pts, n_rows=n))
        return out


class StubCamera:
    """project_batch of CameraHandle's signature: pixel = (x, y) / z + 5 * slot, a flag for every point with x == 0."""

    def __init__(self):
        self.calls = []

    def project_batch(self, items):
        self.calls.append([it.get("slot") for it in items])
        out = []
        for it in items:
            p = np.asarray(it["points"], dtype=np.float64).reshape(-1, 3)
            pix = p[:, :2] / p[:, 2:3] + 5.0 * (it.get("slot") or 0)
            out.append(dict(pixels=pix, flags=(p[:, 0] == 0).astype(np.uint8)))
        return out


POSES, EXT, NXT = np.zeros((11, 7)), np.zeros(7), np.ones(7)


def test_batch_is_two_calls_and_each_item_is_predict_pixels(vio):
    fe = vio.frontend
    items = [dict(frame_count=10, poses=POSES, ext=EXT, fm_slot=0),
             dict(frame_count=9, poses=POSES, ext=EXT, next_pose=NXT, fm_slot=2, camera_slot=3),
             dict(frame_count=10, poses=POSES, ext=EXT, fm_slot=5, camera_slot=1, width=20, height=12)]
    fm, cam = StubFm(), StubCamera()
    got = fe.predict_pixels_batch(fm, cam, items, width=14, height=9)
    assert len(fm.calls) == 1 and len(cam.calls) == 1 and len(got) == 3
    assert fm.calls[0] == [(0, 10, False), (2, 9, True), (5, 10, False)] and cam.calls[0] == [None, 3, 1]
    for it, (ids, pix) in zip(items, got):
        fm1, cam1 = StubFm(), StubCamera()
        w_ids, w_pix = fe.predict_pixels(fm1, cam1, it["frame_count"], POSES, EXT, next_pose=it.get("next_pose"), fm_slot=it["fm_slot"],
                                         camera_slot=it.get("camera_slot"), width=it.get("width", 14), height=it.get("height", 9))
        assert len(fm1.calls) == 1 and len(cam1.calls) == 1           # the one-item case of the same two calls
        assert ids.dtype == w_ids.dtype and np.array_equal(ids, w_ids) and pix.dtype == w_pix.dtype and pix.tobytes() == w_pix.tobytes()
    # the filters did something: a flagged point and pixels outside the image left, and the third item's own size kept more
    assert 0 not in got[0][0] and len(got[0][0]) < 3 and len(got[2][0]) > len(got[0][0])
    free = fe.predict_pixels_batch(StubFm(), StubCamera(), items[:1])[0]
    assert len(free[0]) == 2                                             # without a size only the flag filters


def test_an_empty_batch_still_makes_the_two_calls(vio):
    fm, cam = StubFm(), StubCamera()
    assert vio.frontend.predict_pixels_batch(fm, cam, []) == [] and fm.calls == [[]] and cam.calls == [[]]


class StubFrames:
    """What BatchFeatureTracker asks of a frame.FrameHandle, recorded."""

    def __init__(self, info=None):
        self.calls, self.info = [], info or {}

    def set_config(self, **kw):
        self.calls.append(("set_config", kw))

    def set_tracker(self, **kw):
        self.calls.append(("set_tracker", kw))

    def set_prediction_fallback(self, k):
        self.calls.append(("set_prediction_fallback", k))

    def set_prediction_batch(self, items):
        self.calls.append(("set_prediction_batch", [(s, np.array(i), np.array(p)) for s, i, p in items]))

    def read_predict_info(self, slot):
        self.calls.append(("read_predict_info", slot))
        return dict(dict(n_listed=9, n_guessed=4, n_ok_guessed=2, fell_back=True), **self.info.get(slot, {}))

    def read_batch(self, imgs, t, slots=None, publish=True):
        self.calls.append(("read_batch", list(slots)))
        return [dict(pts=np.zeros((0, 2), np.float32), ids=np.zeros(0, np.int64), track_cnt=np.zeros(0, np.int32),
                     un_pts=np.zeros((0, 2), np.float32), velocity=np.zeros((0, 2), np.float32)) for _ in slots]


IMG = np.zeros((12, 16), dtype=np.uint8)


def names(fr):
    return [c[0] for c in fr.calls]


def test_without_a_prediction_the_handle_sees_the_calls_it_saw_before(vio):
    fr = StubFrames()
    bt = vio.BatchFeatureTracker(fr, [3, 1])
    assert names(fr) == ["set_config", "set_tracker"]
    bt.read_images([IMG, IMG], 0.0)
    bt.set_predictions({})
    bt.read_images([IMG, IMG], 1.0)
    assert names(fr) == ["set_config", "set_tracker", "read_batch", "read_batch"]
    assert bt.pred_info == [dict(n_guessed=0, fell_back=False)] * 2


@pytest.mark.parametrize("prediction,want", [(dict(min_tracked=10), 10), (dict(), 0)])
def test_prediction_arms_the_fallback_on_the_handle(vio, prediction, want):
    fr = StubFrames()
    vio.BatchFeatureTracker(fr, [0], prediction=prediction)
    assert ("set_prediction_fallback", want) in fr.calls


def test_set_predictions_is_one_call_for_the_next_read_only(vio):
    fr = StubFrames({1: dict(n_guessed=7, fell_back=False)})
    bt = vio.BatchFeatureTracker(fr, [3, 1, 8])
    bt.set_predictions({1: ([5, 6], [[1.5, 2.5], [3.5, 4.5]]), 3: ([], np.zeros((0, 2)))})
    sent = [c for c in fr.calls if c[0] == "set_prediction_batch"]
    assert len(sent) == 1 and sorted(s for s, _, _ in sent[0][1]) == [1, 3]
    by = {s: (i, p) for s, i, p in sent[0][1]}
    assert by[1][0].tolist() == [5, 6] and np.asarray(by[1][1]).tolist() == [[1.5, 2.5], [3.5, 4.5]] and len(by[3][0]) == 0
    bt.read_images([IMG] * 3, 0.0)
    assert names(fr)[-3:] == ["read_batch", "read_predict_info", "read_predict_info"]
    assert sorted(c[1] for c in fr.calls[-2:]) == [1, 3]
    # one dict per slot, in the order of `slots`, with FeatureTracker.pred_info's keys
    assert bt.pred_info == [dict(n_guessed=4, fell_back=True), dict(n_guessed=7, fell_back=False), dict(n_guessed=0, fell_back=False)]
    assert set(bt.pred_info[0]) == set(vio.FeatureTracker(None, None).pred_info)
    n = len(fr.calls)
    bt.read_images([IMG] * 3, 1.0)                                       # the read after: nothing of the prediction is left
    assert names(fr)[n:] == ["read_batch"] and bt.pred_info == [dict(n_guessed=0, fell_back=False)] * 3


def test_set_predictions_checks_its_slots(vio):
    fr = StubFrames()
    bt = vio.BatchFeatureTracker(fr, [0, 1])
    with pytest.raises(ValueError, match="slot 7"):
        bt.set_predictions({7: ([1], [[0.0, 0.0]])})
    assert "set_prediction_batch" not in names(fr)
