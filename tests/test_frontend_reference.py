"""frontend.FeatureTracker (readImage and updateID restated) over the numpy restatements of the tracker and the detector
(tests/flow_reference.py, tests/detect_reference.py): the fixture pair, then image 1 again as a third frame.  check_frames holds the
invariants; tests/test_gpu_detect.py runs the same over the two GPU handles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_CNT, MIN_DIST = 150, 30


class Tracker:
    """flow_reference.multi_level behind FlowHandle's interface."""

    def track(self, img_prev, img_next, pts, guess=None):
        out, st, its, cost = fr.multi_level(img_prev, img_next, pts, guess, inverse=1)
        return dict(next_pts=out, status=st, iterations=its, cost=cost)


def fixture_frames():
    a = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
    b = np.load(os.path.join(GOLDEN, "flow_image_2.npz"))["image"]
    return [a, b, a]


def pairwise_ok(pts, min_dist):
    c = np.rint(pts.astype(np.float64)).astype(np.int64)
    d = np.sum((c[:, None, :] - c[None, :, :]) ** 2, axis=2)
    d[np.arange(len(c)), np.arange(len(c))] = min_dist ** 2
    return bool(np.all(d >= min_dist ** 2))


def check_frames(ft, frames, max_cnt=MAX_CNT, min_dist=MIN_DIST):
    """Runs the frames through ft and holds every frame to the invariants; returns the frames' outputs (ids after update_ids)."""
    outs, known = [], {}
    for t, img in enumerate(frames):
        before = dict(zip(ft.ids.tolist(), ft.track_cnt.tolist()))
        out = ft.read_image(img, float(t))
        n, n_new = len(out["pts"]), ft.n_new
        assert out["pts"].shape == (n, 2) and out["ids"].shape == (n,) and out["track_cnt"].shape == (n,)
        assert n <= max_cnt and n > 0
        # new points enter last, with id -1 and count 1; the survivors' counts grew by one
        assert np.all(out["ids"][n - n_new:] == -1) and np.all(out["track_cnt"][n - n_new:] == 1)
        assert np.all(out["ids"][:n - n_new] >= 0)
        for i, c in zip(out["ids"][:n - n_new].tolist(), out["track_cnt"][:n - n_new].tolist()):
            assert c == before[i] + 1, (t, i)
        assert np.all(out["track_cnt"][:n - n_new][1:] <= out["track_cnt"][:n - n_new][:-1])       # setMask's order
        assert pairwise_ok(out["pts"], min_dist)
        h, w = img.shape
        r = np.rint(out["pts"].astype(np.float64))
        assert np.all((r[:, 0] >= 0) & (r[:, 0] < w) & (r[:, 1] >= 0) & (r[:, 1] < h))
        ids = ft.update_ids()
        assert len(set(ids.tolist())) == n and np.all(ids >= 0)
        assert np.array_equal(ids[:n - n_new], out["ids"][:n - n_new])                              # ids are stable
        assert np.array_equal(ids[n - n_new:], len(known) + np.arange(n_new))                       # ... and new ones are the next free
        for i in ids[n - n_new:].tolist():
            known[i] = t
        outs.append(dict(pts=out["pts"], ids=ids, track_cnt=out["track_cnt"], n_new=n_new))
    return outs


@pytest.fixture(scope="module")
def vio_pkg(vio):
    return vio


def test_fixture_sequence(vio_pkg):
    frames = fixture_frames()
    ft = vio_pkg.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST)
    outs = check_frames(ft, frames)
    first = dr.detect(frames[0])
    assert outs[0]["n_new"] == first["n_new"] and np.array_equal(outs[0]["pts"], first["new_pts"])
    # most of the first frame's corners are followed through the sequence
    assert np.sum(outs[1]["track_cnt"] == 2) >= 0.8 * first["n_new"]
    assert np.sum(outs[2]["track_cnt"] == 3) >= 0.7 * first["n_new"]
    assert ft.n_id == sum(o["n_new"] for o in outs)


def test_unpublished_frame_detects_nothing(vio_pkg):
    frames = fixture_frames()
    calls = []

    class CountingDetector(dr.Detector):
        def detect(self, *a, **kw):
            calls.append(1)
            return dr.Detector.detect(self, *a, **kw)

    ft = vio_pkg.FeatureTracker(Tracker(), CountingDetector(), max_cnt=40, min_dist=MIN_DIST)
    a = ft.read_image(frames[0], 0.0)
    ids_a = ft.update_ids()
    b = ft.read_image(frames[1], 1.0, publish=False)
    assert len(calls) == 1 and ft.n_new == 0
    assert 0 < len(b["pts"]) <= len(a["pts"]) and set(b["ids"].tolist()) <= set(ids_a.tolist())
    assert np.all(b["track_cnt"] == 2)
    # a tracker that never published has nothing to follow
    empty = vio_pkg.FeatureTracker(Tracker(), CountingDetector()).read_image(frames[0], 0.0, publish=False)
    assert len(empty["pts"]) == 0 and len(calls) == 1


def test_reject_hook(vio_pkg):
    frames = fixture_frames()
    seen = []

    def reject(cur, forw):
        seen.append((cur.copy(), forw.copy()))
        keep = np.ones(len(cur), dtype=bool)
        keep[::2] = False
        return keep

    ft = vio_pkg.FeatureTracker(Tracker(), dr.Detector(), max_cnt=40, min_dist=MIN_DIST, reject=reject)
    a = ft.read_image(frames[0], 0.0)
    ids_a = ft.update_ids()
    assert not seen                                              # (nothing was tracked yet)
    b = ft.read_image(frames[1], 1.0)
    ft.update_ids()
    assert len(seen) == 1
    cur, forw = seen[0]
    assert cur.shape == forw.shape and len(cur) > 0
    # the pairs are matched: cur rows are first-frame points in their order, forw their tracked positions, close by in this sequence
    idx = [int(np.nonzero(np.all(a["pts"] == c, axis=1))[0][0]) for c in cur]
    assert idx == sorted(idx) and np.all(np.abs(forw - cur) < 20)
    dropped = set(ids_a[idx][::2].tolist())
    kept = set(ids_a[idx][1::2].tolist())
    survivors = set(b["ids"][b["ids"] >= 0].tolist())
    assert not (dropped & survivors) and survivors <= kept
