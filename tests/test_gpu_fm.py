"""libvio_fm_hip (include/vio_fm.h) on the device against tests/fm_reference.py: every integer, id, flag and point
byte-equal; parallax_sum bit-equal to the device-order sum and the keyframe decision equal to the reference-order one; untriangulated
inverse depths and shifted depths bit-equal to the restatement, shifted depths inside the forward error bound of the reference's;
triangulated depths within TRI_RTOL of the golden and of vio_triangulate.  Shapes: the smallest at which a kernel can go wrong (a
wavefront, a chunk of 1024 rows, the full table of 2048), see each test."""
import os

import numpy as np
import pytest

import fm_reference as fr
import fm_util as fu
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TRI_RTOL = 1e-7                                          # tests/test_feature_manager_golden.py's figure for the same data
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048]  # a wavefront is 64 rows, the workgroup (one chunk) 1024, the table 2048
BAD_ARG = -1


@pytest.fixture(scope="module")
def fh(vio):
    h = vio.load_fm().create()                           # (a missing library raises: a failure, not a skip)
    yield h
    h.close()


@pytest.fixture(scope="module")
def fmz():
    return np.load(os.path.join(GOLDEN_DIR, "feature_manager.npz"))


def make_tracks(seed, n, depth_known=0.5, start_max=10):
    """n tracks of every (start, n_obs) a window can hold, ids distinct, not ascending, some above 2^31."""
    rng = np.random.RandomState(seed)
    ids = rng.permutation(n).astype(np.int64) * 2500013 + 11
    out = []
    for i in range(n):
        start = int(rng.randint(0, start_max + 1))
        k = int(rng.randint(1, 12 - start))
        depth = float(rng.uniform(2.0, 9.0)) if rng.uniform() < depth_known else -1.0
        out.append(dict(id=int(ids[i]), start=start, depth=depth, flag=int(rng.randint(0, 2)), pts=rng.uniform(-0.7, 0.7, (k, 2))))
    return out


def seed_slot(fh, slot, tracks):
    fh.tracks_set(slot, *fr.tracks_to_arrays(tracks))
    assert fh.counts(slot) == fr.counts(tracks)


def slot_tracks(fh, slot):
    return fr.arrays_to_tracks(fh.tracks_get(slot))


def check_slot(fh, slot, want, res=None):
    fr.assert_tracks_equal(slot_tracks(fh, slot), want)
    assert fh.counts(slot) == fr.counts(want)
    if res is not None:
        assert (res["n_tracks"], res["n_landmarks"], res["n_observations"]) == fr.counts(want)


def poses_of(vio):
    from test_triangulate import make_tracks as tri_tracks
    return tri_tracks(vio, 1, seed=1)[3:5]


def cam_poses(vio, poses, ext):
    R = [vio.synth.quat_to_rot(poses[k, 3:7]) for k in range(11)]
    ric, tic = vio.synth.quat_to_rot(ext[3:7]), ext[0:3]
    return [R[k] @ ric for k in range(11)], [poses[k, 0:3] + R[k] @ tic for k in range(11)]


# ------------------------------------------------ the table ---------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_tracks_round_trip(fh, n):
    tracks = make_tracks(n, n)
    seed_slot(fh, 0, tracks)
    check_slot(fh, 0, tracks)


def test_tracks_set_refuses_and_writes_nothing(vio, fh):
    base = make_tracks(5, 70)
    seed_slot(fh, 0, base)
    t = lambda **kw: dict(dict(id=1, start=0, depth=-1.0, flag=0, pts=np.zeros((2, 2))), **kw)      # noqa: E731
    bad = [make_tracks(1, 2049), [t(pts=np.zeros((12, 2)))], [t(start=-1)], [t(start=9, pts=np.zeros((3, 2)))], [t(id=4), t(id=4)],
           [t(pts=np.array([[0.0, np.nan], [0.0, 0.0]]))], [t(depth=np.inf)]]
    for tracks in bad:
        with pytest.raises(vio.VioError) as e:
            fh.tracks_set(0, *fr.tracks_to_arrays(tracks))
        assert e.value.status == BAD_ARG
        check_slot(fh, 0, base)
    ids, start, depth, flag, off, pts = fr.tracks_to_arrays([t()])
    with pytest.raises(vio.VioError):                    # a track without an observation
        fh.tracks_set(0, ids, start, depth, flag, np.array([0, 0], dtype=np.int64), pts)
    check_slot(fh, 0, base)


# ------------------------------------------------ slide -------------------------------------------------------------------
def slide_args(vio, kind, behind=False):
    poses, ext = poses_of(vio)
    Rc, tc = cam_poses(vio, poses, ext)
    if kind == fr.BACK_SHIFT_DEPTH:
        return (0, Rc[0], tc[0], -Rc[1] if behind else Rc[1], tc[1])
    return (fu.WINDOW_SIZE if kind == fr.FRONT else 0, None, None, None, None)


@pytest.mark.parametrize("kind", [fr.BACK_SHIFT_DEPTH, fr.BACK, fr.FRONT])
@pytest.mark.parametrize("n", ROWS)
def test_slide_matches_the_restatement(vio, fh, kind, n):
    tracks = make_tracks(100 + n, n)
    seed_slot(fh, 1, tracks)
    args = slide_args(vio, kind)
    res = fh.slide_batch([(1, kind) + args])[0]
    assert res["status"] == 0
    check_slot(fh, 1, fr.slide(tracks, kind, *args), res)


@pytest.mark.parametrize("kind", [fr.BACK_SHIFT_DEPTH, fr.BACK, fr.FRONT])
def test_slide_erasures_at_wavefront_and_chunk_edges(vio, fh, kind):
    """The erased rows are the first and the last of a wavefront and of a chunk, and their neighbours stay."""
    tracks = make_tracks(7, 2048)
    edges = [0, 63, 64, 127, 1023, 1024, 1087, 2047]
    for r, t in enumerate(tracks):
        erase = r in edges
        if kind == fr.FRONT:                             # one observation, at frame 9: erased; neighbours: not seen at frame 9
            t["start"], t["pts"] = (9, t["pts"][:1]) if erase else (min(t["start"], 7), t["pts"][:1])
        else:
            k = 2 if kind == fr.BACK_SHIFT_DEPTH else 1
            t["start"], t["pts"] = (0, np.resize(t["pts"], (k, 2))) if erase else (max(t["start"], 1), t["pts"][:min(len(t["pts"]), 11 - max(t["start"], 1))])
    seed_slot(fh, 1, tracks)
    args = slide_args(vio, kind)
    res = fh.slide_batch([(1, kind) + args])[0]
    want = fr.slide(tracks, kind, *args)
    assert len(want) == 2048 - len(edges) and {t["id"] for t in tracks} - {t["id"] for t in want} == {tracks[r]["id"] for r in edges}
    check_slot(fh, 1, want, res)


def test_back_shift_depth_one_and_two_observations_left(vio, fh):
    tracks = make_tracks(9, 130, depth_known=1.0)
    for r, t in enumerate(tracks):
        t["start"] = 0
        t["pts"] = np.resize(t["pts"], (2 + r % 2, 2))     # 2 observations: 1 left, erased; 3: 2 left, kept and re-hosted
    seed_slot(fh, 1, tracks)
    args = slide_args(vio, fr.BACK_SHIFT_DEPTH)
    res = fh.slide_batch([(1, fr.BACK_SHIFT_DEPTH) + args])[0]
    want = fr.slide(tracks, fr.BACK_SHIFT_DEPTH, *args)
    assert len(want) == 65 and all(len(t["pts"]) == 2 for t in want)
    check_slot(fh, 1, want, res)                         # (the shifted depths bit-equal to the restatement)


def test_back_shift_depth_behind_the_new_host_gives_init_depth(vio, fh):
    """new_R = -R: every re-hosted point has dep_j <= 0 (the golden's behind_camera, at a full table)."""
    tracks = make_tracks(13, 2048, depth_known=1.0)
    seed_slot(fh, 1, tracks)
    args = slide_args(vio, fr.BACK_SHIFT_DEPTH, behind=True)
    res = fh.slide_batch([(1, fr.BACK_SHIFT_DEPTH) + args])[0]
    want = fr.slide(tracks, fr.BACK_SHIFT_DEPTH, *args)
    moved = {t["id"] for t in tracks if t["start"] == 0 and len(t["pts"]) >= 3}
    assert len(moved) > 50 and all(t["depth"] == fr.INIT_DEPTH for t in want if t["id"] in moved)
    check_slot(fh, 1, want, res)


def test_front_branches(vio, fh):
    """start == frame_count, a track ended before frame_count - 1, a track of one observation."""
    p = lambda k: np.arange(2.0 * k).reshape(k, 2) / 16      # noqa: E731
    tracks = [dict(id=1, start=10, depth=-1.0, flag=0, pts=p(1)),        # start == frame_count: start 9
              dict(id=2, start=3, depth=2.0, flag=1, pts=p(4)),          # ended at 6 < 9: untouched
              dict(id=3, start=9, depth=-1.0, flag=0, pts=p(1)),         # one observation, at frame 9: erased
              dict(id=4, start=9, depth=-1.0, flag=0, pts=p(2)),         # frames 9, 10: loses frame 9
              dict(id=5, start=2, depth=3.0, flag=0, pts=p(9)),          # frames 2 .. 10: loses index 7
              dict(id=6, start=0, depth=3.0, flag=0, pts=p(10))]         # frames 0 .. 9: loses index 9
    seed_slot(fh, 1, tracks)
    res = fh.slide_batch([(1, fr.FRONT, 10)])[0]
    want = fr.slide(tracks, fr.FRONT, 10)
    assert [(t["id"], t["start"], len(t["pts"])) for t in want] == [(1, 9, 1), (2, 3, 4), (4, 9, 1), (5, 2, 8), (6, 0, 9)]
    check_slot(fh, 1, want, res)


# ------------------------------------------------ set_depth ---------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_set_depth_then_remove_failures(fh, n):
    """Negative inverse depths at the first and last usable row of a wavefront and of a chunk, then removeFailures."""
    tracks = make_tracks(200 + n, n, start_max=5)
    nl = fr.counts(tracks)[1]
    x = np.random.RandomState(n).uniform(0.05, 0.5, nl)
    x[[k for k in (0, 63, 64, 127, 1023, 1024, nl - 1) if 0 <= k < nl]] *= -1.0
    seed_slot(fh, 2, tracks)
    res = fh.set_depth_batch([(2, x)], mode=0, remove_failures=False)[0]
    want = fr.set_depth(tracks, x)
    check_slot(fh, 2, want, res)
    seed_slot(fh, 2, tracks)
    res = fh.set_depth_batch([(2, x)], mode=0, remove_failures=True)[0]
    want = fr.remove_failures(want)
    check_slot(fh, 2, want, res)


def test_clear_depth_leaves_the_flags_and_a_wrong_length_is_refused(vio, fh):
    tracks = make_tracks(31, 200, start_max=5)
    nl = fr.counts(tracks)[1]
    x = np.random.RandomState(1).uniform(-0.5, 0.5, nl)
    seed_slot(fh, 2, tracks)
    res = fh.set_depth_batch([(2, x)], mode=1, remove_failures=True)[0]       # (flags untouched: whatever had 2 goes, nothing has)
    want = fr.set_depth(tracks, x, clear=True)
    assert [t["flag"] for t in want] == [t["flag"] for t in tracks]
    check_slot(fh, 2, want, res)
    for bad in (x[:-1], np.concatenate([x, [0.1]]), np.where(np.arange(nl) == 3, np.nan, x)):
        with pytest.raises(vio.VioError) as e:
            fh.set_depth_batch([(2, bad)])
        assert e.value.status == BAD_ARG
        check_slot(fh, 2, want)


# ------------------------------------------------ add ---------------------------------------------------------------------
def ending_at(tracks, fc):
    """The tracks cut so that none reaches past frame fc - 1, the form a table has before frame fc arrives."""
    out = []
    for t in fr.copy_tracks(tracks):
        if t["start"] > fc - 1:
            t["start"] = max(fc - 1, 0)
        t["pts"] = t["pts"][:max(1, min(len(t["pts"]), fc - t["start"]))]
        out.append(t)
    return out


def check_add(fh, slot, tracks, fc, ids, pts):
    seed_slot(fh, slot, tracks)
    res = fh.add_batch([(slot, fc, ids, pts)])[0]
    want, ref = fr.add(tracks, fc, ids, pts)
    for k in ("status", "keyframe", "last_track_num", "parallax_num", "n_new"):
        assert res[k] == ref[k], (k, res, ref)
    assert np.float64(res["parallax_sum"]).tobytes() == np.float64(ref["parallax_sum"]).tobytes()        # the device's order, bit for bit
    check_slot(fh, slot, want, res)
    return res, ref


@pytest.mark.parametrize("n0", ROWS)
@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_add_matched_and_new_interleaved(fh, n0, order):
    fc = 6
    tracks = ending_at(make_tracks(300 + n0, n0), fc)
    rng = np.random.RandomState(n0)
    live = [t["id"] for t in tracks if t["start"] + len(t["pts"]) == fc]
    old = rng.permutation(live)[:min(len(live), 500)]
    n_new = min(300, fr.MAX_TRACKS - n0)
    new = np.arange(n_new, dtype=np.int64) * 2500013 + 1250000                    # between the table's ids; every other one above 2^32
    new[1::2] += 2 ** 32
    ids = np.concatenate([old, new]).astype(np.int64)
    ids = np.sort(ids)[::-1].copy() if order == "descending" else rng.permutation(ids)
    res, ref = check_add(fh, 3, tracks, fc, ids, rng.uniform(-0.7, 0.7, (len(ids), 2)))
    assert res["status"] == 0 and res["last_track_num"] == len(old) and res["n_new"] == len(new)
    if n0 >= 1023:
        assert res["parallax_num"] > 0 and ids.max() > 2 ** 32


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1024])
@pytest.mark.parametrize("matched", ["all", "none"])
def test_add_incoming_sizes(fh, n, matched):
    fc = 4
    rng = np.random.RandomState(n)
    tracks = [dict(id=int(i) * 7 + 1, start=2, depth=-1.0, flag=0, pts=rng.uniform(-0.7, 0.7, (2, 2))) for i in rng.permutation(1024)]
    if matched == "all":
        ids = rng.permutation([t["id"] for t in tracks])[:n]
    else:
        ids = rng.permutation(n).astype(np.int64) * 2500013 + 17
    res, _ = check_add(fh, 3, tracks, fc, ids, rng.uniform(-0.7, 0.7, (n, 2)))
    assert res["status"] == 0 and res["last_track_num"] == (n if matched == "all" else 0)


@pytest.mark.parametrize("last,fc,key_by_gate", [(19, 5, True), (20, 5, False), (30, 1, True), (30, 2, False)])
def test_add_gates(fh, last, fc, key_by_gate):
    """last_track_num 19 and 20, frame_count 1 and 2: on the gate's side keyframe = 1 with parallax_num = 0."""
    rng = np.random.RandomState(last + fc)
    tracks = [dict(id=10 * i + 3, start=0, depth=-1.0, flag=0, pts=rng.uniform(-0.5, 0.5, (fc, 2))) for i in range(40)]
    ids = np.array([t["id"] for t in tracks[:last]] + [5], dtype=np.int64)
    res, _ = check_add(fh, 3, tracks, fc, ids, rng.uniform(-0.5, 0.5, (len(ids), 2)))
    assert res["last_track_num"] == last and (res["parallax_num"] == 0) == key_by_gate
    if key_by_gate:
        assert res["keyframe"] == 1


def test_add_without_a_parallax_row_is_a_keyframe(fh):
    """parallax_num == 0 behind both gates: every matched track began at frame_count - 1."""
    rng = np.random.RandomState(2)
    tracks = [dict(id=i, start=4, depth=-1.0, flag=0, pts=rng.uniform(-0.5, 0.5, (1, 2))) for i in range(30)]
    res, _ = check_add(fh, 3, tracks, 5, np.arange(30), np.zeros((30, 2)))
    assert (res["last_track_num"], res["parallax_num"], res["keyframe"]) == (30, 0, 1)


def test_add_small_and_large_parallax_decide_differently(fh):
    rng = np.random.RandomState(4)
    for step, key in ((0.001, 0), (0.1, 1)):
        p0 = rng.uniform(-0.5, 0.5, (50, 1, 2))
        tracks = [dict(id=i, start=0, depth=-1.0, flag=0, pts=np.concatenate([p0[i], p0[i] + step, p0[i] + 2 * step])) for i in range(50)]
        res, _ = check_add(fh, 3, tracks, 3, np.arange(50), p0[:, 0] + 3 * step)
        assert res["keyframe"] == key and res["parallax_num"] == 50


def test_add_device_rules_leave_the_slot_untouched(fh):
    rng = np.random.RandomState(8)
    full = ending_at(make_tracks(11, 2048), 6)
    live = [t["id"] for t in full if t["start"] + len(t["pts"]) == 6][:40]
    # 2049 rows: 40 matched and one new id
    res, _ = check_add(fh, 3, full, 6, np.array(live + [7], dtype=np.int64), rng.uniform(-1, 1, (41, 2)))
    assert res["status"] == fr.STATUS_TABLE_FULL and res["n_tracks"] == 2048
    res, _ = check_add(fh, 3, full, 6, np.array(live, dtype=np.int64), rng.uniform(-1, 1, (40, 2)))          # ... and without it: fits
    assert res["status"] == 0
    # a matched track with a gap: it ended at frame 3, the image is frame 6
    gap = [dict(id=i, start=1, depth=-1.0, flag=0, pts=rng.uniform(-1, 1, (5 if i != 77 else 3, 2))) for i in range(100)]
    res, _ = check_add(fh, 3, gap, 6, np.arange(100), rng.uniform(-1, 1, (100, 2)))
    assert res["status"] == fr.STATUS_GAP
    res, _ = check_add(fh, 3, gap, 6, np.setdiff1d(np.arange(100), [77]), rng.uniform(-1, 1, (99, 2)))
    assert res["status"] == 0
    # a twelfth observation
    twelve = [dict(id=i, start=0, depth=-1.0, flag=0, pts=rng.uniform(-1, 1, (11 if i == 5 else 10, 2))) for i in range(30)]
    res, _ = check_add(fh, 3, twelve, 10, np.arange(30), rng.uniform(-1, 1, (30, 2)))
    assert res["status"] == fr.STATUS_OBS_FULL


def test_add_host_rules(vio, fh):
    base = make_tracks(3, 10)
    seed_slot(fh, 3, base)
    p = np.zeros((3, 2))
    bad = [(3, 11, [1, 2, 3], p), (3, -1, [1, 2, 3], p), (3, 2, [1, 2, 2], p), (3, 2, [1, 2, 3], np.array([[0, 0], [0, np.inf], [0, 0]])),
           (256, 2, [1, 2, 3], p), (3, 2, np.arange(1025), np.zeros((1025, 2)))]
    for it in bad:
        with pytest.raises(vio.VioError) as e:
            fh.add_batch([it])
        assert e.value.status == BAD_ARG, it
        check_slot(fh, 3, base)


# ------------------------------------------------ export ------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_export_without_triangulation_equals_the_restatement(vio, fh, n):
    """Tracks with and without a depth mixed, triangulate = 0: every array bit-equal (1.0 / -1.0 included)."""
    tracks = make_tracks(400 + n, n)
    seed_slot(fh, 4, tracks)
    poses, ext = poses_of(vio)
    got = fh.export_batch([(4, poses, ext)], triangulate=False)[0]
    want = fr.export(tracks)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
    assert got["n_triangulated"] == 0
    check_slot(fh, 4, tracks, got)


def test_export_triangulates_and_loads_into_a_context(vio, fh, hip_lib):
    """Tracks with and without a depth mixed: the triangulated depths against vio_triangulate on the same inputs, the fallback on the
    same tracks, every other array equal to the restatement's, and the arrays load into a context."""
    from test_triangulate import make_tracks as tri_tracks
    sf, off, pts, poses, ext, d0, _ = tri_tracks(vio, 1300, seed=21, noise=1.5 / 460.0, have_depth_frac=0.5)
    n = len(sf)
    tracks = [dict(id=5 * (n - i), start=int(sf[i]), depth=float(d0[i]), flag=0, pts=pts[off[i]:off[i + 1]]) for i in range(n)]
    seed_slot(fh, 4, tracks)
    got = fh.export_batch([(4, poses, ext)], triangulate=True)[0]
    lib = hip_lib.context().triangulate(sf, off, pts, poses, ext, d0)
    touched = (np.diff(off) >= 2) & (sf < 8) & ~(d0 > 0)
    assert got["n_triangulated"] == int(touched.sum()) > 100
    after = slot_tracks(fh, 4)
    dep = np.array([t["depth"] for t in after])
    np.testing.assert_array_equal(dep == fr.INIT_DEPTH, lib == fr.INIT_DEPTH)
    np.testing.assert_allclose(dep, lib, rtol=TRI_RTOL, atol=0)
    assert dep[~touched].tobytes() == d0[~touched].tobytes()              # a known depth, and a track that is not usable, stay
    want_tracks = [dict(t, depth=float(d)) for t, d in zip(tracks, dep)]
    check_slot(fh, 4, want_tracks, got)
    want = fr.export(want_tracks)
    for k, v in want.items():
        assert got[k].tobytes() == v.tobytes(), k
    ctx = hip_lib.context()
    ctx.set_window(poses, np.zeros((11, 9)), ext)
    ctx.set_landmarks(got["inv_depth"])                  # (_ck raises unless VIO_OK)
    ctx.set_observations(got["lm"], got["host"], got["target"], got["pts_i"], got["pts_j"])
    again = fh.export_batch([(4, poses, ext)], triangulate=True)[0]      # every depth is known now
    assert again["n_triangulated"] == 0 and again["inv_depth"].tobytes() == got["inv_depth"].tobytes()


@pytest.mark.parametrize("k", range(4))
def test_triangulated_depths_match_the_golden_and_vio_triangulate(fh, hip_lib, fmz, k):
    p = "tri%d_" % k
    z = fmz
    n = len(z[p + "start"])
    init = float(z[p + "init_depth"])
    fh.set_config(init_depth=init)
    try:
        fh.tracks_set(4, np.arange(n), z[p + "start"], z[p + "depth_in"], np.zeros(n, dtype=np.int32), z[p + "off"], z[p + "pts"])
        res = fh.export_batch([(4, z[p + "poses"], z[p + "ext"])], triangulate=True)[0]
    finally:
        fh.set_config()
    got = fh.tracks_get(4)["depth"]
    want = z[p + "depth_out"]
    np.testing.assert_array_equal(got == init, want == init)             # the < 0.1 rule fires on the same tracks
    np.testing.assert_allclose(got, want, rtol=TRI_RTOL, atol=0)
    lib = hip_lib.context().triangulate(z[p + "start"], z[p + "off"], z[p + "pts"], z[p + "poses"], z[p + "ext"], z[p + "depth_in"], init_depth=init)
    np.testing.assert_allclose(got, lib, rtol=TRI_RTOL, atol=0)
    touched = (np.diff(z[p + "off"]) >= 2) & (z[p + "start"] < 8) & ~(z[p + "depth_in"] > 0)
    assert res["n_triangulated"] == int(touched.sum())
    np.testing.assert_array_equal(got[~touched], z[p + "depth_in"][~touched])
    print("tri%d: %d of %d triangulated depths bit-equal to vio_triangulate" % (k, int((got[touched] == lib[touched]).sum()), int(touched.sum())))


# ------------------------------------------------ corresponding -----------------------------------------------------------
@pytest.mark.parametrize("n", [0, 65, 1025, 2048])
@pytest.mark.parametrize("l,r", [(0, 10), (9, 10), (4, 4), (3, 8)])
def test_corresponding_matches_the_restatement(fh, n, l, r):
    tracks = make_tracks(500 + n, n)
    seed_slot(fh, 5, tracks)
    got = fh.corresponding_batch([(5, l, r)])[0]
    want = fr.corresponding(tracks, l, r)
    assert got["n_rows"] == len(want) and got["rows"].tobytes() == want.tobytes()
    check_slot(fh, 5, tracks, got)


def test_corresponding_without_a_spanning_track(vio, fh):
    tracks = [t for t in make_tracks(6, 300) if not (t["start"] <= 2 and t["start"] + len(t["pts"]) - 1 >= 9)]
    seed_slot(fh, 5, tracks)
    got = fh.corresponding_batch([(5, 2, 9)])[0]
    assert got["n_rows"] == 0 and got["rows"].shape == (0, 4)
    with pytest.raises(vio.VioError):
        fh.corresponding_batch([(5, 5, 4)])


# ------------------------------------------------ golden replays ----------------------------------------------------------
def apply_op_on_device(fh, slot, op, poses, ext):
    c = op[0]
    if c == 1:
        return fh.export_batch([(slot, poses, ext)], triangulate=True)[0]
    if c in (2, 7):
        return fh.set_depth_batch([(slot, op[1])], mode=0 if c == 2 else 1)[0]
    if c == 3:                                           # removeFailures alone: clearDepth with the depths as they are erases nothing else
        x = fh.export_batch([(slot, poses, ext)], triangulate=False)[0]["inv_depth"]
        return fh.set_depth_batch([(slot, x)], mode=1, remove_failures=True)[0]
    if c == 4:
        return fh.slide_batch([(slot, fr.BACK_SHIFT_DEPTH, 0) + tuple(op[1:5])])[0]
    if c == 5:
        return fh.slide_batch([(slot, fr.BACK)])[0]
    return fh.slide_batch([(slot, fr.FRONT, op[1])])[0]


@pytest.mark.parametrize("name", fu.SCENARIOS)
def test_golden_scenarios_on_the_device(fh, fmz, name):
    p = "sc_%s_" % name
    tracks = fr.copy_tracks(fu.arrays_to_tracks(fmz, p + "in_"))
    ops = fu.arrays_to_ops(fmz, p + "op_")
    seed_slot(fh, 6, tracks)
    has_tri = False
    for op in ops:
        apply_op_on_device(fh, 6, op, fmz[p + "poses"], fmz[p + "ext"])
        tracks = fr.apply_op(tracks, op, fmz[p + "poses"], fmz[p + "ext"])
        has_tri = has_tri or op[0] == 1
        if not has_tri:
            check_slot(fh, 6, tracks)                    # bit-equal to the restatement as long as nothing was triangulated
    got, want = slot_tracks(fh, 6), fu.arrays_to_tracks(fmz, p + "out_")
    src = {t["id"]: t for t in fu.arrays_to_tracks(fmz, p + "in_")}
    shift = [o for o in ops if o[0] == 4]
    assert len(got) == len(want) and fh.counts(6)[1] == int(fmz[p + "count"])
    for g, w in zip(got, want):
        assert (g["id"], g["start"], g["flag"]) == (w["id"], w["start"], w["flag"]) and np.array_equal(g["pts"], w["pts"])
        if has_tri:
            np.testing.assert_allclose(g["depth"], w["depth"], rtol=TRI_RTOL)
        elif shift and src[g["id"]]["start"] == 0 and w["depth"] != fr.INIT_DEPTH:
            s = src[g["id"]]
            assert abs(g["depth"] - w["depth"]) <= fr.shift_depth_bound(s["pts"][0][0], s["pts"][0][1], s["depth"], *shift[0][1:5])
        else:
            assert g["depth"] == w["depth"]
    if name == "behind_camera":
        assert sum(w["depth"] == fr.INIT_DEPTH and src[w["id"]]["start"] == 0 for w in want) > 0


def replay_on_device(fh, slot, z, p):
    fh.reset(slot)
    keys, lasts, tracks = [], [], []
    for f in range(len(z[p + "frame_count"])):
        lo, hi = z[p + "off"][f], z[p + "off"][f + 1]
        fc = int(z[p + "frame_count"][f])
        res = fh.add_batch([(slot, fc, z[p + "ids"][lo:hi], z[p + "pts"][lo:hi])])[0]
        tracks, ref = fr.add(tracks, fc, z[p + "ids"][lo:hi], z[p + "pts"][lo:hi])
        assert res["status"] == 0 and res["parallax_num"] == ref["parallax_num"]
        assert np.float64(res["parallax_sum"]).tobytes() == np.float64(ref["parallax_sum"]).tobytes()
        keys.append(res["keyframe"])
        lasts.append(res["last_track_num"])
        if fc == fu.WINDOW_SIZE:
            kind = fr.BACK if res["keyframe"] else fr.FRONT
            fh.slide_batch([(slot, kind, fu.WINDOW_SIZE)])
            tracks = fr.slide(tracks, kind, fu.WINDOW_SIZE)
    return keys, lasts


def test_golden_parallax_sequence_on_the_device(fh, fmz):
    keys, lasts = replay_on_device(fh, 6, fmz, "par_")
    np.testing.assert_array_equal(keys, fmz["par_key"])
    np.testing.assert_array_equal(lasts, fmz["par_last_track_num"])
    fr.assert_tracks_equal(slot_tracks(fh, 6), fr.copy_tracks(fu.arrays_to_tracks(fmz, "par_out_")))


def test_large_golden_sequence_on_the_device(fh):
    z = np.load(os.path.join(GOLDEN_DIR, "fm_large.npz"))
    keys, lasts = replay_on_device(fh, 6, z, "seq_")
    np.testing.assert_array_equal(keys, z["seq_key"])
    np.testing.assert_array_equal(lasts, z["seq_last_track_num"])
    want = fr.arrays_to_tracks(dict(ids=z["seq_out_id"], start=z["seq_out_start"], depth=z["seq_out_depth"], flag=z["seq_out_flag"],
                                    off=z["seq_out_off"], pts=z["seq_out_pts"]))
    assert len(want) > 1024
    fr.assert_tracks_equal(slot_tracks(fh, 6), want)


# ------------------------------------------------ batches -----------------------------------------------------------------
def history(vio, fh, slots, seeds, break_seed=None):
    """One history per slot, every step one batched call for all of them.  What a slot sees depends on its seed alone (not on its
    position in the call or its slot index); returns each slot's final table and the log of its results."""
    poses, ext = poses_of(vio)
    Rc, tc = cam_poses(vio, poses, ext)
    for s in slots:
        fh.reset(s)
    log = [[] for _ in slots]
    rngs = [np.random.RandomState(77 + seed) for seed in seeds]
    cur = [np.arange(90 + 25 * seed, dtype=np.int64) * 3 + seed for seed in seeds]
    nxt = [int(c.max()) + 3 for c in cur]
    for fc in range(0, 7):
        items = []
        for i, (s, seed) in enumerate(zip(slots, seeds)):
            rng = rngs[i]
            ids = rng.permutation(cur[i])
            pts = rng.uniform(-0.6, 0.6, (len(ids), 2)) * (0.01 if (fc // 2 + seed) % 2 else 1.0)
            # (a slot whose frame was refused keeps being refused: its tracks end where they did)
            items.append((s, 3 if seed == break_seed and fc == 5 else fc, ids, pts))
            lost = rng.uniform(size=len(ids)) < 0.1                        # a lost track's id never comes back
            fresh = nxt[i] + 3 * np.arange(int(lost.sum()), dtype=np.int64)
            cur[i] = np.concatenate([ids[~lost], fresh])
            nxt[i] += 3 * int(lost.sum())
        for i, r in enumerate(fh.add_batch(items)):
            log[i].append((r["status"], r["keyframe"], r["last_track_num"], r["parallax_num"], r["parallax_sum"], r["n_new"]))
    exp = fh.export_batch([(s, poses, ext) for s in slots])
    for i, r in enumerate(exp):
        log[i].append((r["n_triangulated"], r["inv_depth"].tobytes(), r["lm"].tobytes(), r["target"].tobytes()))
    xs = [np.where(np.arange(len(r["inv_depth"])) % (3 + seed) == 0, -0.2, 0.2) for seed, r in zip(seeds, exp)]
    fh.set_depth_batch(list(zip(slots, xs)), remove_failures=True)
    kinds = [fr.BACK_SHIFT_DEPTH, fr.BACK, fr.FRONT, fr.BACK_SHIFT_DEPTH, fr.BACK]
    fh.slide_batch([(s, kinds[seed % 5], 6, Rc[0], tc[0], Rc[1], tc[1]) for s, seed in zip(slots, seeds)])
    for i, r in enumerate(fh.corresponding_batch([(s, 1, 4) for s in slots])):
        log[i].append(r["rows"].tobytes())
    return [fh.tracks_get(s) for s in slots], log


def same_tables(a, b):
    return len(a) == len(b) and all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in x)


def test_five_slots_in_one_call_equal_each_alone_and_in_other_slots(vio, fh):
    seeds = [0, 1, 2, 3, 4]
    tabs, log = history(vio, fh, [10, 11, 12, 13, 14], seeds)
    assert len({len(t["ids"]) for t in tabs}) == 5 and all(len(t["ids"]) > 64 for t in tabs)
    assert all(e[0] == 0 for lg in log for e in lg[:7]) and {e[1] for lg in log for e in lg[2:7]} == {0, 1}
    tabs2, log2 = history(vio, fh, [200, 3, 255, 17, 64], seeds)         # other slot indices
    assert same_tables(tabs, tabs2) and log == log2
    tabs3, log3 = history(vio, fh, [14, 13, 12, 11, 10], seeds[::-1])    # the same sequences again, at other positions of the call
    assert same_tables(tabs, tabs3[::-1]) and log == log3[::-1]
    for i in range(5):                                                   # each alone
        t1, l1 = history(vio, fh, [30 + i], [seeds[i]])
        assert same_tables([tabs[i]], t1) and log[i] == l1[0]


def test_one_slot_breaking_a_device_rule_does_not_touch_the_others(vio, fh):
    seeds = [0, 1, 2, 3, 4]
    tabs, log = history(vio, fh, [20, 21, 22, 23, 24], seeds)
    tabs_b, log_b = history(vio, fh, [20, 21, 22, 23, 24], seeds, break_seed=2)
    assert log_b[2][5][0] == fr.STATUS_GAP and log_b[2][:5] == log[2][:5]
    for i in (0, 1, 3, 4):
        assert same_tables([tabs[i]], [tabs_b[i]]) and log[i] == log_b[i]
    assert not same_tables([tabs[2]], [tabs_b[2]])


def test_a_slot_listed_twice_is_refused_with_nothing_changed(vio, fh):
    a, b = make_tracks(1, 100), make_tracks(2, 70)
    seed_slot(fh, 40, a)
    seed_slot(fh, 41, b)
    poses, ext = poses_of(vio)
    calls = [lambda: fh.add_batch([(40, 3, [1], np.zeros((1, 2))), (41, 3, [1], np.zeros((1, 2))), (40, 3, [2], np.zeros((1, 2)))]),
             lambda: fh.slide_batch([(40, fr.BACK), (40, fr.BACK)]),
             lambda: fh.export_batch([(41, poses, ext), (41, poses, ext)]),
             lambda: fh.corresponding_batch([(40, 0, 1), (41, 0, 1), (41, 0, 1)]),
             lambda: fh.set_depth_batch([(40, np.ones(fr.counts(a)[1])), (40, np.ones(fr.counts(a)[1]))])]
    for call in calls:
        with pytest.raises(vio.VioError) as e:
            call()
        assert e.value.status == BAD_ARG and "twice" in str(e.value)
        check_slot(fh, 40, a)
        check_slot(fh, 41, b)


def test_reset_then_reuse(fh):
    seed_slot(fh, 50, make_tracks(1, 1500))
    fh.reset(50)
    assert fh.counts(50) == (0, 0, 0) and slot_tracks(fh, 50) == []
    rng = np.random.RandomState(0)
    ids = rng.permutation(200).astype(np.int64)
    res, _ = check_add(fh, 50, [], 0, ids, rng.uniform(-1, 1, (200, 2)))
    assert res["n_new"] == 200 and [t["id"] for t in slot_tracks(fh, 50)] == list(range(200))         # appended in ascending id order


def test_batch_feature_manager_takes_feature_frames_as_they_are(vio, fh):
    """frontend.BatchFeatureTracker.feature_frames()'s pairs: int64 ids, (n, 7) rows whose first two columns came from float32."""
    fm = vio.BatchFeatureManager(fh, slots=[60, 61])
    for s in fm.slots:
        fh.reset(s)
    rng = np.random.RandomState(5)
    tracks = [[], []]
    for fc in range(3):
        frames = []
        for i in range(2):
            n = 150
            rows = np.zeros((n, 7))
            rows[:, 0:2] = rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
            rows[:, 2] = 1.0
            frames.append((np.arange(n, dtype=np.int64) + 2 ** 33, rows))
        res = fm.add_feature_frames(frames, [fc, fc])
        for i in range(2):
            tracks[i], ref = fr.add(tracks[i], fc, frames[i][0], frames[i][1][:, 0:2])
            assert res[i]["keyframe"] == ref["keyframe"]
    poses, ext = poses_of(vio)
    wins = fm.windows([poses, poses], ext, triangulate=False)
    for i in range(2):
        check_slot(fh, fm.slots[i], tracks[i])
        assert wins[i]["pts_j"].tobytes() == fr.export(tracks[i])["pts_j"].tobytes() and len(wins[i]["inv_depth"]) == 150
    fm.set_depths([np.full(150, 0.2), np.where(np.arange(150) % 2, -0.2, 0.2)])
    assert [fh.counts(s)[0] for s in fm.slots] == [150, 75]
    fm.slide([vio.fm.BACK, vio.fm.FRONT], frame_counts=[0, 2])
    assert [r["n_rows"] for r in fm.corresponding(0, 1)] == [150, 75]
