"""frontend.FeatureTracker with a rejecter (rejectWithF and undistortedPoints restated, tests/reject_reference.py) on the fixture
sequence of tests/test_frontend_reference.py: un_pts, velocity and feature_frame() against a plain-Python walk over the frames, and
rejecter=None gives what it gave before there was one.  tests/test_gpu_reject.py runs the same over the three GPU handles."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import reject_reference as rr  # noqa: E402
from test_frontend_reference import MAX_CNT, MIN_DIST, Tracker, check_frames, fixture_frames  # noqa: E402

DT = 0.05


def run(ft, frames):
    """Every frame's dict (ids after update_ids) and feature_frame()."""
    outs = []
    for t, img in enumerate(frames):
        out = ft.read_image(img, DT * t)
        out["ids_after"] = ft.update_ids()
        out["feature_frame"] = ft.feature_frame() if ft.rejecter is not None else None
        outs.append(out)
    return outs


def walk(cam, outs):
    """undistortedPoints and the publisher restated frame by frame in plain Python on the tracker's pts / ids / track_cnt."""
    prev = {}                                                # id at the time -> the float32 normalised point
    res = []
    for t, o in enumerate(outs):
        un = cam.lift(o["pts"]).astype(np.float32)
        vel = np.zeros_like(un)
        cur = {}
        for k, i in enumerate(o["ids"].tolist()):            # (the ids before update_ids: -1 for the new points)
            cur.setdefault(i, un[k])
            if i != -1 and i in prev and t > 0:
                vel[k] = ((un[k].astype(np.float64) - prev[i].astype(np.float64)) / (DT * t - DT * (t - 1))).astype(np.float32)
        prev = cur
        rows = [(int(o["ids_after"][k]), [un[k, 0], un[k, 1], 1.0, o["pts"][k, 0], o["pts"][k, 1], vel[k, 0], vel[k, 1]])
                for k in range(len(un)) if o["track_cnt"][k] > 1]
        res.append((un, vel, rows))
    return res


def test_un_pts_velocity_and_feature_frame(vio):
    cam = rr.Camera(**rr.EUROC)
    frames = fixture_frames() + [fixture_frames()[1]]
    ft = vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=rr.Rejecter(cam))
    outs = run(ft, frames)
    nonzero = 0
    for t, (o, (un, vel, rows)) in enumerate(zip(outs, walk(cam, outs))):
        assert o["un_pts"].dtype == np.float32 and o["un_pts"].tobytes() == un.tobytes(), t
        assert o["velocity"].dtype == np.float32 and o["velocity"].tobytes() == vel.tobytes(), t
        ids, ff = o["feature_frame"]
        assert ids.dtype == np.int64 and ff.dtype == np.float64 and ff.shape == (len(rows), 7)
        assert ids.tolist() == [r[0] for r in rows] and np.array_equal(ff, np.array([r[1] for r in rows], dtype=np.float64).reshape(-1, 7))
        assert np.all(ids >= 0) and len(set(ids.tolist())) == len(ids)
        nonzero += int(np.any(vel != 0, axis=1).sum())
        if t == 0:
            assert len(ids) == 0                             # (every point is new: nothing is published, System.cpp:236)
    assert nonzero > 50                                      # from the third frame on the old tracks move
    assert len(outs[2]["feature_frame"][0]) > 50


def test_rejecter_sees_matched_pairs_and_the_frame_count(vio):
    cam = rr.Camera(**rr.EUROC)
    calls = []

    class Spy(rr.Rejecter):
        def reject(self, cur, forw, pair=0):
            keep = rr.Rejecter.reject(self, cur, forw, pair)
            calls.append((len(cur), pair, keep.copy()))
            return keep

    frames = fixture_frames()
    ft = vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=Spy(cam))
    outs = check_frames(ft, frames)                          # the tracker's invariants hold with a rejecter
    assert [c[1] for c in calls] == [1, 2] and all(c[0] >= 8 for c in calls)
    # the static fixture scene moves rigidly: almost every pair is kept, and what is dropped leaves the tracker
    for (n, _, keep), o in zip(calls, outs[1:]):
        assert keep.mean() >= 0.8
        assert np.sum(o["track_cnt"] > 1) <= keep.sum()


def test_without_a_rejecter_nothing_changes(vio):
    """rejecter=None gives the dict FeatureTracker gave before it took a rejecter: tests/golden/frontend_fixture.npz was recorded with
    that FeatureTracker (tests/golden/make_golden_frontend.py)."""
    frames = fixture_frames()
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_fixture.npz"))
    for kw in ({}, dict(rejecter=None)):
        outs = run(vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST, **kw), frames)
        for t, o in enumerate(outs):
            assert set(o) == {"pts", "ids", "track_cnt", "ids_after", "feature_frame"} and o["feature_frame"] is None
            for k in ("pts", "ids", "track_cnt", "ids_after"):
                g = gold["%s_%d" % (k, t)]
                assert o[k].dtype == g.dtype and o[k].shape == g.shape and o[k].tobytes() == g.tobytes(), (t, k)
    assert len(gold["pts_2"]) > 100 and np.sum(gold["track_cnt_2"] == 3) > 50          # (the recording is not trivial)
    ft = vio.FeatureTracker(Tracker(), dr.Detector())
    ft.read_image(frames[0], 0.0)
    try:
        ft.feature_frame()
    except RuntimeError:
        pass
    else:
        raise AssertionError("feature_frame without a rejecter must raise")
