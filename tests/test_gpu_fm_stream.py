"""include/vio_fm_stream.h on the device: vio_fm_init_depth_batch against a twin slot that is cleared and exported
with triangulation (the depth in front of the product is k_fm_export's bit for bit), vio_fm_tracks_batch against vio_fm_tracks_get
byte for byte, and stream drivers that keep their FeatureManager in a slot (StreamDriver(features=...)) beside the same drivers with
their tracks / depth dicts."""
import numpy as np
import pytest

import fm_reference as fr
import fm_stream_reference as fsr
from test_gpu_fm import TRI_RTOL, seed_slot
from test_stream import same_stops

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 255, 256, 257, 1025, 2048]                 # k_fm_init_depth walks chunks of 256 rows, k_fm_tracks of 1024; the table has 2048
SCALES = [0.37, 1.0, 2.0006]
BAD_ARG = -1


@pytest.fixture(scope="module")
def fh(vio):
    h = vio.load_fm().create()                           # (a missing library raises: a failure, not a skip)
    yield h
    h.close()


_tables = {}


def table(vio, n, seed=0):
    """n rows, usable and unusable mixed: three in four are tracks of one point seen from the poses (half of them hold a positive depth
    already, which the hand-over must not keep), one in four has random points, which triangulate to anything: some below 0.1.
    Returns (tracks, poses, ext with tic = 0).  Made once per (n, seed)."""
    if (n, seed) not in _tables:
        from test_triangulate import make_tracks as tri_tracks
        n_geo = n - n // 4
        sf, off, pts, poses, ext, d0, _ = tri_tracks(vio, n_geo, seed=100 + n + seed, noise=1.5 / 460.0, have_depth_frac=0.5)
        tracks = [dict(id=7 * (n - i) + 3, start=int(sf[i]), depth=float(d0[i]), flag=i % 3, pts=pts[off[i]:off[i + 1]]) for i in range(n_geo)]
        rng = np.random.RandomState(n + 17 * seed)
        for i in range(n // 4):
            start = int(rng.randint(0, 11))
            k = int(rng.randint(1, 12 - start))
            depth = float(rng.uniform(2.0, 9.0)) if rng.uniform() < 0.5 else -1.0
            tracks.append(dict(id=2 ** 33 + i, start=start, depth=depth, flag=int(rng.randint(0, 3)), pts=rng.uniform(-0.7, 0.7, (k, 2))))
        order = rng.permutation(n)
        _tables[(n, seed)] = ([tracks[i] for i in order], poses, np.concatenate([np.zeros(3), ext[3:7]]))
    tracks, poses, ext0 = _tables[(n, seed)]
    return fr.copy_tracks(tracks), poses.copy(), ext0.copy()


def twin_depths(fh, slot, tracks, poses, ext0):
    """What k_fm_export writes for every usable row once its depth is cleared: the twin of the hand-over's triangulation."""
    seed_slot(fh, slot, tracks)
    nl = fr.counts(tracks)[1]
    fh.set_depth_batch([(slot, -np.ones(nl))], mode=1)                   # DEPTH_CLEAR: 1.0 / -1.0
    res = fh.export_batch([(slot, poses, ext0)], triangulate=True)[0]
    assert res["n_triangulated"] == nl
    return fh.tracks_get(slot)["depth"]


def arrays_equal(a, b):
    for k in ("ids", "start", "depth", "flag", "off", "pts"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------ init_depth_batch --------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_init_depth_is_the_export_kernels_depth_times_s(vio, fh, n):
    tracks, poses, ext0 = table(vio, n)
    us = np.array([fr.usable(t) for t in tracks], dtype=bool)
    before = fsr.tracks_arrays(tracks)
    twin = twin_depths(fh, 9, tracks, poses, ext0)
    if n >= 255:
        assert (twin[us] == fr.INIT_DEPTH).sum() > 0 and (before["depth"][us] > 0).sum() > n // 8 and (~us).sum() > 0
    for s in SCALES:
        seed_slot(fh, 8, tracks)
        res = fh.init_depth_batch([(8, poses, ext0, s)])[0]
        got = fh.tracks_get(8)
        want = dict(before, depth=np.where(us, twin * np.float64(s), before["depth"]))
        arrays_equal(got, want)                                          # the unusable rows, the flags and every point as they were
        assert res["status"] == 0 and res["n_triangulated"] == int(us.sum())
        assert (res["n_tracks"], res["n_landmarks"], res["n_observations"]) == fr.counts(tracks) == fh.counts(8)
    t = fh.timing()
    assert all(np.isfinite(v) and v >= 0 for v in t.values())


def test_init_depth_five_slots_in_one_call_equal_each_alone_and_in_other_slots(vio, fh):
    sizes, scales = [3, 257, 1025, 64, 700], [0.37, 1.0, 2.0006, 11.5, 0.002]
    tabs = [table(vio, n, seed=1) for n in sizes]
    for i, (tr, _, _) in enumerate(tabs):
        seed_slot(fh, 10 + i, tr)
        seed_slot(fh, 200 - 7 * i, tr)
    res = fh.init_depth_batch([(10 + i, p, e, s) for i, ((_, p, e), s) in enumerate(zip(tabs, scales))])
    for i, ((tr, p, e), s) in enumerate(zip(tabs, scales)):
        alone = fh.init_depth_batch([(200 - 7 * i, p, e, s)])[0]
        assert alone == res[i]
        arrays_equal(fh.tracks_get(10 + i), fh.tracks_get(200 - 7 * i))
        seed_slot(fh, 200 - 7 * i, tr)                                   # a repeated call is bitwise identical
        assert fh.init_depth_batch([(200 - 7 * i, p, e, s)])[0] == alone
        arrays_equal(fh.tracks_get(10 + i), fh.tracks_get(200 - 7 * i))


def test_init_depth_argument_rules(vio, fh):
    tracks, poses, ext0 = table(vio, 257)
    seed_slot(fh, 8, tracks)
    seed_slot(fh, 9, tracks)
    before = fsr.tracks_arrays(tracks)

    def refused(items, text):
        with pytest.raises(vio.VioError) as e:
            fh.init_depth_batch(items)
        assert e.value.status == BAD_ARG and text in str(e.value), str(e.value)
        arrays_equal(fh.tracks_get(8), before)
        arrays_equal(fh.tracks_get(9), before)
    refused([(8, poses, ext0, 1.5), (9, poses, ext0, 1.5), (8, poses, ext0, 1.5)], "item 2: slot 8 is listed twice")
    for s in (0.0, -1.0, float("nan"), float("inf")):
        refused([(8, poses, ext0, 1.5), (9, poses, ext0, s)], "item 1: s must be finite and > 0")
    bad = poses.copy()
    bad[4, 5] = np.inf
    refused([(8, poses, ext0, 1.5), (9, bad, ext0, 1.5)], "item 1: a pose is not finite")
    refused([(8, poses, ext0, 1.5), (256, poses, ext0, 1.5)], "slot 256 outside")
    assert fh.init_depth_batch([]) == []


# ------------------------------------------------ tracks_batch ------------------------------------------------------------
def full_table():
    rng = np.random.RandomState(5)
    return [dict(id=3 * i + 1, start=0, depth=float(i + 1), flag=i % 3, pts=rng.uniform(-0.7, 0.7, (11, 2))) for i in range(fr.MAX_TRACKS)]


def test_tracks_batch_is_tracks_get_byte_for_byte(vio, fh):
    tabs = [table(vio, n)[0] for n in ROWS] + [full_table()]
    slots = [30 + 9 * i for i in range(len(tabs))]
    for s, tr in zip(slots, tabs):
        seed_slot(fh, s, tr)
    res = fh.tracks_batch(slots)
    for s, tr, r in zip(slots, tabs, res):
        arrays_equal(r, fh.tracks_get(s))
        arrays_equal(r, fsr.tracks_arrays(tr))
        assert r["status"] == 0 and r["n_rows"] == sum(len(t["pts"]) for t in tr)
        assert (r["n_tracks"], r["n_landmarks"], r["n_observations"]) == fr.counts(tr)
    assert res[-1]["n_rows"] == 22528
    for k in (4, 7, 2):                                                   # a slot's result depends neither on the batch nor on the order
        alone = fh.tracks_batch([slots[k]])[0]
        arrays_equal(alone, res[k])
        assert {f: alone[f] for f in ("status", "n_tracks", "n_rows")} == {f: res[k][f] for f in ("status", "n_tracks", "n_rows")}
    again = fh.tracks_batch(slots[::-1])[::-1]
    for a, r in zip(again, res):
        arrays_equal(a, r)
    assert all(np.isfinite(v) and v >= 0 for v in fh.timing().values())


def test_tracks_batch_capacity_is_a_device_rule(vio, fh):
    tr, _, _ = table(vio, 257)
    nb, _, _ = table(vio, 1025)
    total = sum(len(t["pts"]) for t in tr)
    seed_slot(fh, 40, tr)
    seed_slot(fh, 41, nb)
    fh.reset(42)
    for caps in (dict(cap_tracks=[257, 1025, 0], cap_obs=[total - 1, 1025 * 11, 0]), dict(cap_tracks=[256, 1025, 0], cap_obs=[total, 1025 * 11, 0])):
        res = fh.tracks_batch([40, 41, 42], **caps)
        assert res[0]["status"] == vio.fm.STATUS_CAPACITY == 4 and res[0]["n_rows"] == total and res[0]["n_tracks"] == 257
        for k in ("ids", "start", "depth", "flag", "off", "pts"):
            assert not res[0][k].any(), k                                # nothing written
        assert res[1]["status"] == 0
        arrays_equal(res[1], fh.tracks_get(41))                          # the neighbour is served
        assert res[2]["status"] == 0 and res[2]["n_rows"] == 0 and list(res[2]["off"]) == [0] and len(res[2]["ids"]) == 0      # an empty slot too
    exact = fh.tracks_batch([40], cap_tracks=[257], cap_obs=[total])[0]
    arrays_equal(exact, fh.tracks_get(40))
    arrays_equal(fh.tracks_get(40), fsr.tracks_arrays(tr))               # the slot is as it was
    with pytest.raises(vio.VioError) as e:
        fh.tracks_batch([40, 40])
    assert e.value.status == BAD_ARG and "listed twice" in str(e.value)


# ------------------------------------------------ drivers -----------------------------------------------------------------
STREAMS = [(0, 0, 16), (1, 4, 18), (2, 3, 20)]          # seed, nonkey_every, frames


def run_group(vio, hip_lib, fm=None, est=None, **kw):
    from vio_amd import batch_stream, stream as vs
    drivers, sh = [], None
    for k, (seed, nonkey, n_frames) in enumerate(STREAMS):
        extra = dict(kw)
        if sh is not None:
            extra["ctx_kwargs"] = dict(stream=sh)
        if fm is not None:
            extra["features"] = (fm, 5 + 50 * k)
        if est is not None:
            extra["state"] = (est, 3 + 100 * k)
        drivers.append(vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=n_frames, seed=seed), triangulate=True, nonkey_every=nonkey, **extra))
        sh = drivers[0].ctx.get_stream()
    records = [fsr.record_dict_driver(d) for d in drivers] if fm is None else None
    trajs = batch_stream.run_batched(drivers, vio.load_marg().create(stream=sh))
    return drivers, trajs, records


def compare_groups(vio, plain, with_fm, fm):
    (dp, tp, want), (dd, td, _) = plain, with_fm
    worst = 0.0
    for k, (a, b) in enumerate(zip(dp, dd)):
        got = fm.exports[b.fm_slot]
        assert len(got) == len(want[k]) == 2 * len(tp[k])
        for step, (g, w) in enumerate(zip(got, want[k])):
            for f in ("feature_ids", "lm", "host", "target", "pts_i", "pts_j"):
                assert g[f].dtype == w[f].dtype and np.array_equal(g[f], w[f]), (k, step, f)
        np.testing.assert_allclose(got[0]["inv_depth"], want[k][0]["inv_depth"], rtol=TRI_RTOL)      # two triangulation kernels
        assert a.flags == b.flags and not hasattr(b, "tracks") and not hasattr(b, "depth")
        gt = a.ground_truth()
        diff = np.abs(td[k][:, 1:4] - tp[k][:, 1:4]).max()
        worst = max(worst, diff)
        assert diff < 1e-3
        ate_p, ate_d = vio.stream.ate_rmse(tp[k], gt), vio.stream.ate_rmse(td[k], gt)
        assert abs(ate_d - ate_p) <= 0.01 * ate_p
        same_stops(b.reports, a.reports)
    return worst


def test_drivers_with_features_follow_the_dict_path(vio, hip_lib, fh):
    """Three drivers through run_batched with their FeatureManagers in slots: the index arrays and the points of every window are the
    dict path's, the trajectories are held to test_stream.py's bar between two implementations, and a frame makes one call of each
    kind for the drivers still running."""
    plain = run_group(vio, hip_lib)
    fm = fsr.Recording(fh)
    with_fm = run_group(vio, hip_lib, fm=fm)
    worst = compare_groups(vio, plain, with_fm, fm)
    print("features= against the dict path: largest position difference %.3g m" % worst)
    calls = fm.calls[33:]                                                # (the constructors' eleven adds each)
    assert fm.calls[:33] == [("add_batch", 1)] * 33
    frames = [len(t) for t in with_fm[1]]
    active = [sum(f > i for f in frames) for i in range(max(frames))]
    assert [n for c, n in calls if c == "export_batch"] == [a for a in active for _ in (0, 1)]
    assert [n for c, n in calls if c == "set_depth_batch"] == active
    assert [n for c, n in calls if c == "slide_batch"] == [n for c, n in calls if c == "add_batch"] == [sum(f > i + 1 for f in frames) for i in range(max(frames) - 1)]
    assert {c for c, _ in calls} == {"export_batch", "set_depth_batch", "slide_batch", "add_batch"}


def test_drivers_with_features_and_state(vio, hip_lib, fh):
    """The same three with their window states in estimator-state slots as well: the slide's four arrays are the slot's."""
    est = vio.load_est().create()
    try:
        plain = run_group(vio, hip_lib, est=est)
        fm = fsr.Recording(fh)
        with_fm = run_group(vio, hip_lib, fm=fm, est=est)
        worst = compare_groups(vio, plain, with_fm, fm)
        print("features= with state= against state= alone: largest position difference %.3g m" % worst)
    finally:
        est.close()


def test_initial_group_initialises_through_the_slots(vio, hip_lib, fh):
    """Two drivers in the INITIAL state with sfm=True: one tracks_batch gives both windows' sfm_f, the tries succeed as they do on the
    dict path, one init_depth_batch hands the depths over (init_apply's numpy lines within TRI_RTOL: two triangulation kernels), and
    the group runs to the end."""
    from vio_amd import batch_stream, stream as vs

    def group(fm):
        ds, sh = [], None
        for k, seed in enumerate((3, 4)):
            kw = dict(ctx_kwargs=dict(stream=sh)) if sh is not None else {}
            if fm is not None:
                kw["features"] = (fm, 60 + k)
            ds.append(vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=15, landmarks_per_frame=60, track_len=10, seed=seed, pixel_noise=0.1 / 460.0),
                                      seed=2, triangulate=True, initialize=dict(sfm=True), **kw))
            sh = ds[0].ctx.get_stream()
        return ds, sh
    plain, _ = group(None)
    fm = fsr.Recording(fh)
    drv, sh = group(fm)
    del fm.calls[:]
    assert batch_stream.initialize_batched(plain) == 1 and batch_stream.initialize_batched(drv) == 1
    assert fm.calls == [("tracks_batch", 2), ("init_depth_batch", 2)]
    for a, b in zip(plain, drv):
        assert a.initialized and b.initialized and a.init_tries == b.init_tries == 1
        assert b.init_result["s"] == a.init_result["s"] and b.n_triangulated == a.n_triangulated
        assert np.array_equal(a.have_depth, b.have_depth) and a.have_depth.sum() > 100
        np.testing.assert_allclose(b.inv_depth[b.have_depth], a.inv_depth[a.have_depth], rtol=TRI_RTOL)
    tb = batch_stream.run_batched(drv, vio.load_marg().create(stream=sh))
    ta = [d.run() for d in plain]
    for x, y in zip(ta, tb):
        assert len(x) == len(y) == 5 and np.abs(x[:, 1:4] - y[:, 1:4]).max() < 1e-3


def test_driver_without_features_is_untouched(vio, hip_lib):
    """Without features= the driver takes the lines it took before: features=None and no argument give the same trajectory bit for
    bit, and the driver keeps its dicts."""
    from vio_amd import stream as vs
    a = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=5), triangulate=True, nonkey_every=3)
    b = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=5), triangulate=True, nonkey_every=3, features=None)
    assert a.fm is None and b.fm is None and hasattr(a, "tracks") and hasattr(b, "depth")
    assert np.array_equal(a.run(), b.run()) and a.fm_keyframe == []
