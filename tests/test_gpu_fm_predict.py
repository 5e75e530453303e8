"""vio_fm_predict_batch (include/vio_fm_predict.h, k_fm_predict) on the device against
tests/fm_predict_reference.py: the ids and the points byte for byte, no tolerance, n_rows and the three counts.  Tables
(tests/predict_inputs.py, whose properties tests/test_predict_inputs_cpu.py asserts) are seeded with tracks_set and read back with
tracks_get: the call writes nothing to them.  Shapes: the wavefront edges of the ballot scan (63, 64, 65), the chunk edge of FM_NT
(1023, 1024, 1025) and the full table; frame counts 0, 1, 2 and 10; the next pose given and not."""
import ctypes as C

import numpy as np
import pytest

import fm_predict_reference as fp
import predict_inputs as pi

pytestmark = pytest.mark.gpu
BAD_ARG = -1
FIELDS = ("ids", "start", "depth", "flag", "off", "pts")


@pytest.fixture(scope="module")
def fh(vio):
    h = vio.load_fm().create()                           # (a missing library raises: a failure, not a skip)
    yield h
    h.close()


def seed(fh, slot, t):
    fh.tracks_set(slot, *[t[k] for k in FIELDS])
    assert fh.counts(slot)[0] == len(t["ids"])


def unmoved(fh, slot, t):
    got = fh.tracks_get(slot)
    for k in FIELDS:
        assert np.asarray(got[k]).tobytes() == np.asarray(t[k]).astype(np.asarray(got[k]).dtype).tobytes(), k


def counts_of(t):
    nobs = t["off"][1:] - t["off"][:-1]
    us = (nobs >= 2) & (t["start"] < 8)
    return len(nobs), int(us.sum()), int((nobs[us] - 1).sum())


def same(res, t, fc, poses, ext, nxt, name):
    ids, pts, _, _ = fp.predict(t, fc, poses, ext, nxt)
    assert res["status"] == 0 and res["n_rows"] == len(ids), (name, res["n_rows"], len(ids))
    assert np.array_equal(res["ids"], ids), name
    assert res["pts_cam"].shape == pts.shape and res["pts_cam"].tobytes() == pts.tobytes(), \
        (name, "%d of %d coordinates differ" % (int(np.sum(res["pts_cam"] != pts)), pts.size))
    assert (res["n_tracks"], res["n_landmarks"], res["n_observations"]) == counts_of(t), name
    assert [res[k] for k in ("keyframe", "last_track_num", "parallax_num", "n_new", "n_triangulated")] == [0] * 5 and res["parallax_sum"] == 0.0
    return len(ids)


@pytest.mark.parametrize("n", pi.SIZES)
@pytest.mark.parametrize("given", [False, True])
def test_every_size_against_the_restatement(fh, n, given):
    poses, ext, nxt = pi.poses(n)
    t, kinds = pi.table(n, 10)
    seed(fh, 5, t)
    nx = nxt if given else None
    res = fh.predict_batch([(5, 10, poses, ext, nx)])[0]
    rows = same(res, t, 10, poses, ext, nx, "n %d" % n)
    assert rows == int(np.sum(kinds == pi.QUALIFIES))
    again = fh.predict_batch([(5, 10, poses, ext, nx)])[0]
    assert again["ids"].tobytes() == res["ids"].tobytes() and again["pts_cam"].tobytes() == res["pts_cam"].tobytes()
    unmoved(fh, 5, t)


@pytest.mark.parametrize("fc", pi.FRAME_COUNTS)
def test_frame_counts(fh, fc):
    poses, ext, nxt = pi.poses(40 + fc)
    t, kinds = pi.table(1025, max(fc, 1)) if fc != 10 else pi.table(65, 10)
    seed(fh, 9, t)
    for nx in (None, nxt):
        res = fh.predict_batch([(9, fc, poses, ext, nx)])[0]
        rows = same(res, t, fc, poses, ext, nx, "frame_count %d" % fc)
        assert (rows == 0) == (fc < 2)
    if fc == 1:                                             # rows that satisfy the three conditions at 1: still nothing
        assert np.any(kinds == pi.QUALIFIES)
    # the table of frame_count 2 asked at 10 and at 1: other rows qualify, or none
    if fc == 2:
        for other in (1, 3, 10):
            same(fh.predict_batch([(9, other, poses, ext, None)])[0], t, other, poses, ext, None, "table of 2 at %d" % other)
    unmoved(fh, 9, t)


@pytest.mark.parametrize("every", [True, False])
def test_all_rows_and_none(fh, every):
    poses, ext, _ = pi.poses(3)
    t = pi.all_or_none(1025, 10, every)
    seed(fh, 0, t)
    res = fh.predict_batch([(0, 10, poses, ext, None)])[0]
    assert same(res, t, 10, poses, ext, None, "every %s" % every) == (1025 if every else 0)
    unmoved(fh, 0, t)


def test_edge_depths(fh):
    poses, ext, _ = pi.poses(2)
    t = pi.edge_depths(5)
    seed(fh, 1, t)
    res = fh.predict_batch([(1, 5, poses, ext, None)])[0]
    assert same(res, t, 5, poses, ext, None, "edge depths") == 3 and np.array_equal(res["ids"], t["ids"][3:])
    assert np.all(np.isfinite(res["pts_cam"]))


def test_six_slots_in_one_call_each_as_alone(fh):
    poses = {s: pi.poses(s) for s, _, _ in pi.SIX}
    tabs = {}
    for s, n, fc in pi.SIX:
        tabs[s] = pi.table(n, fc, seed=s)[0]
        seed(fh, s, tabs[s])
    items = [(s, fc, poses[s][0], poses[s][1], poses[s][2] if s % 2 else None) for s, _, fc in pi.SIX]
    outs = fh.predict_batch(items)
    for it, o in zip(items, outs):
        same(o, tabs[it[0]], it[1], it[2], it[3], it[4], "slot %d" % it[0])
        alone = fh.predict_batch([it])[0]
        assert alone["ids"].tobytes() == o["ids"].tobytes() and alone["pts_cam"].tobytes() == o["pts_cam"].tobytes() and alone["n_rows"] == o["n_rows"]
    back = fh.predict_batch(items[::-1])[::-1]
    assert [(o["ids"].tobytes(), o["pts_cam"].tobytes()) for o in back] == [(o["ids"].tobytes(), o["pts_cam"].tobytes()) for o in outs]
    assert sum(o["n_rows"] > 0 for o in outs) >= 4
    # one table in another slot number: the same bytes
    s0, n0, fc0 = pi.SIX[3]
    seed(fh, 100, tabs[s0])
    a = fh.predict_batch([(100, fc0, poses[s0][0], poses[s0][1], None)])[0]
    b = fh.predict_batch([(s0, fc0, poses[s0][0], poses[s0][1], None)])[0]
    assert a["pts_cam"].tobytes() == b["pts_cam"].tobytes() and a["ids"].tobytes() == b["ids"].tobytes()
    for s in tabs:
        unmoved(fh, s, tabs[s])


def test_a_slot_never_used_predicts_nothing(vio):
    h = vio.load_fm().create()
    try:
        poses, ext, _ = pi.poses(0)
        res = h.predict_batch([(17, 10, poses, ext, None)])[0]
        assert res["status"] == 0 and res["n_rows"] == 0 and res["n_tracks"] == 0 and len(res["ids"]) == 0
    finally:
        h.close()


def test_argument_errors_write_nothing(fh, vio):
    lib = fh.lib
    Item, Res = vio.fm.VioFmPredictItem, vio.fm.VioFmResult
    poses, ext, nxt = pi.poses(0)
    t, _ = pi.table(65, 10)
    seed(fh, 2, t)
    bad_pose, bad_next = poses.copy(), nxt.copy()
    bad_pose[4, 2], bad_next[5] = np.nan, np.inf

    def call(slot=2, fc=10, cap=65, p=poses, e=ext, nx=None, ids_null=False, count=1, twice=False):
        ids, pts = np.full(65, 77, dtype=np.int64), np.full((65, 3), 7.5)
        it = Item(slot, fc, cap, 0, None if p is None else p.ctypes.data, None if e is None else e.ctypes.data, None if nx is None else nx.ctypes.data,
                  None if ids_null else ids.ctypes.data, pts.ctypes.data)
        items = (Item * 2)(it, it)
        res = (Res * 2)()
        res[0].n_rows = res[1].n_rows = 99
        st = lib.fn["predict_batch"](fh.h, C.c_int32(2 if twice else count), C.addressof(items), C.addressof(res))
        return st, np.all(ids == 77) and np.all(pts == 7.5) and res[0].n_rows == 99 and res[1].n_rows == 99

    for kw in (dict(cap=64), dict(fc=-1), dict(fc=11), dict(slot=-1), dict(slot=256), dict(p=None), dict(e=None), dict(p=bad_pose), dict(nx=bad_next),
               dict(ids_null=True), dict(count=-1), dict(count=257), dict(twice=True)):
        st, untouched = call(**kw)
        assert st == BAD_ARG and untouched, kw
    assert call(cap=64)[0] == BAD_ARG and "64 rows" in fh.last_error()
    st, untouched = call()
    assert st == 0 and not untouched
    unmoved(fh, 2, t)
