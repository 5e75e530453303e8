"""rejectWithF and undistortedPoints on the GPU (include/vio_reject.h) against the numpy restatement (tests/reject_reference.py).

The lift, un_pts and velocity are elementwise arithmetic in a fixed order: they are equal to the restatement in every bit, without
tolerance.  The RANSAC must give the restatement's status, winning hypothesis, inlier count and mask exactly.  Its sums follow the
restatement's only to rounding (numpy sums in its own order), so every case asserts on the restatement that no error of the winner,
before or after the refit, lies within 1e-6 (relative) of the gate: `margin`.  The scene seeds were picked on the CPU so that the
restatement alone satisfies this; the smallest margin over every case of this file is 1.1e-3 (n = 4096), the next 3.8e-3 (the winner in
the last round of 65), every other above 3e-2.  F is
held to 10x the restatement's own spread when every virtual pixel the fit reads moves by one ulp (two such perturbations, measured in
the test), plus 1e-13 of its size: the rule of tests/test_gpu_sfm.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reject_reference as rr  # noqa: E402
from test_frontend_reference import MAX_CNT, MIN_DIST, check_frames, fixture_frames  # noqa: E402

pytestmark = pytest.mark.gpu
ROUND, THREADS, CHUNK = 64, 256, 1024            # (asserted against the binding in test_constants)
MIN_MARGIN = 1e-6
_cache = {}


@pytest.fixture(scope="module")
def reject_lib(vio, hip_lib):
    return vio.load_reject()


@pytest.fixture()
def rh(reject_lib):
    h = reject_lib.create()
    h.set_camera(**rr.EUROC)
    yield h
    h.close()


def euroc():
    return rr.Camera(**rr.EUROC)


def test_constants(vio):
    from vio_amd import reject
    assert (reject.ROUND, reject.THREADS, reject.ID_CHUNK, reject.MAX_POINTS) == (ROUND, THREADS, CHUNK, 4096) == (rr.ROUND, rr.THREADS, rr.ID_CHUNK, rr.MAX_POINTS)


# ---- lift, un_pts, velocity: every bit -----------------------------------------------------------------------
def pixels(n, cam, seed=1):
    rng = np.random.RandomState(seed + n)
    return (rng.uniform(0, 1, (n, 2)) * np.array([cam.width - 1, cam.height - 1])).astype(np.float32)


CAMERAS = [("euroc", rr.EUROC), ("simulation", dict(fx=460.0, fy=460.0, cx=320.0, cy=240.0, width=640, height=480))]


@pytest.mark.parametrize("name,params", CAMERAS)
def test_lift_every_bit(reject_lib, name, params):
    cam = rr.Camera(**params)
    h = reject_lib.create()
    h.set_camera(**params)
    corners = np.array([[0, 0], [cam.width - 1, 0], [0, cam.height - 1], [cam.width - 1, cam.height - 1]], dtype=np.float32)
    assert h.lift(corners).tobytes() == cam.lift(corners).tobytes()
    for n in (0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 4096):
        p = pixels(n, cam)
        got = h.lift(p)
        assert got.shape == (n, 2) and got.dtype == np.float64 and got.tobytes() == cam.lift(p).tobytes(), (name, n)
        un, vel = h.undistort(p)
        assert un.dtype == np.float32 and un.tobytes() == rr.un_points(cam, p).tobytes(), (name, n)
        assert vel.shape == (n, 2) and not vel.any()
    assert h.lift(pixels(300, cam)).tobytes() == h.lift(pixels(300, cam)).tobytes()
    h.close()


@pytest.mark.parametrize("m", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 4096])
def test_id_lookup_every_bit(rh, m):
    cam = euroc()
    rng = np.random.RandomState(40 + m)
    n = 300
    pts = pixels(n, cam, seed=2)
    prev_ids = rng.permutation(10 * max(m, 1))[:m].astype(np.int64) + 5
    prev_un = rr.un_points(cam, pixels(m, cam, seed=3))
    ids = rng.randint(5, 10 * max(m, 1) + 5, n).astype(np.int64)          # most ids are unmatched
    ids[::7] = -1
    if m > 0:
        if m > 3:
            prev_ids[m // 3] = prev_ids[0]                                # a repeated id: the first match counts
        ids[8:40] = prev_ids[rng.randint(0, m, 32)]
        ids[1], ids[2] = prev_ids[0], prev_ids[m - 1]                     # the match at the first and at the last entry
        ids[3] = prev_ids[m // 2]
        # on the restatement's side: the last entry's id is there once, so point 2 matches at index m - 1 (for m = CHUNK + 1 that is
        # the one entry of the tail chunk), and point 1 matches at index 0 although its id is repeated at m // 3
        assert np.nonzero(prev_ids == ids[2])[0].tolist() == [m - 1] and int(np.nonzero(prev_ids == ids[1])[0][0]) == 0
        assert m <= 3 or np.nonzero(prev_ids == ids[1])[0].tolist() == [0, m // 3]
    want_un, want_vel = rr.undistort(cam, pts, ids, prev_ids, prev_un, dt=0.05)
    un, vel = rh.undistort(pts, ids, prev_ids, prev_un, 0.05)
    assert un.tobytes() == want_un.tobytes() and vel.dtype == np.float32 and vel.tobytes() == want_vel.tobytes()
    if m > 0:
        assert np.any(want_vel[1] != 0) and np.any(want_vel[2] != 0) and not want_vel[0].any()
        last = ((want_un[2].astype(np.float64) - prev_un[m - 1].astype(np.float64)) / 0.05).astype(np.float32)
        first = ((want_un[1].astype(np.float64) - prev_un[0].astype(np.float64)) / 0.05).astype(np.float32)
        assert want_vel[2].tobytes() == last.tobytes() and want_vel[1].tobytes() == first.tobytes()
    # in a batch, and again: the same bytes
    items = [dict(pts=pts, ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un, dt=0.05), dict(pts=pts[:0], ids=ids[:0]),
             dict(pts=pts[:65], ids=ids[:65], prev_ids=prev_ids, prev_un_pts=prev_un, dt=0.1)]
    a, b = rh.undistort_batch(items), rh.undistort_batch(items)
    assert a[0]["velocity"].tobytes() == want_vel.tobytes() and a[0]["un_pts"].tobytes() == want_un.tobytes()
    assert a[1]["un_pts"].shape == (0, 2) and a[1]["status"] == rr.OK
    assert a[2]["velocity"].tobytes() == rr.undistort(cam, pts[:65], ids[:65], prev_ids, prev_un, dt=0.1)[1].tobytes()
    for x, y in zip(a, b):
        assert x["un_pts"].tobytes() == y["un_pts"].tobytes() and x["velocity"].tobytes() == y["velocity"].tobytes()


def test_undistort_not_finite(rh):
    cam = euroc()
    pts = pixels(10, cam)
    bad = pts.copy()
    bad[4, 0] = np.inf
    ids = np.arange(10, dtype=np.int64)
    out = rh.undistort_batch([dict(pts=pts, ids=ids), dict(pts=bad, ids=ids), dict(pts=pts, ids=ids)])
    assert [o["status"] for o in out] == [rr.OK, rr.NOT_FINITE, rr.OK]
    assert np.isnan(out[1]["un_pts"]).all() and np.isnan(out[1]["velocity"]).all()
    assert out[0]["un_pts"].tobytes() == out[2]["un_pts"].tobytes() == rr.un_points(cam, pts).tobytes()


# ---- RANSAC --------------------------------------------------------------------------------------------------
def scene(n, seed, noise_px=0.1, outlier_share=0.2):
    key = ("scene", n, seed, noise_px, outlier_share)
    if key not in _cache:
        cur, forw, planted, _ = rr.two_view_scene(euroc(), seed=seed, n=n, noise_px=noise_px, outlier_share=outlier_share)
        _cache[key] = (cur, forw)
    return _cache[key]


def collinear_pair():
    x = np.arange(8, dtype=np.float32) * 40 + 100
    y = np.full(8, 200, dtype=np.float32)
    return np.stack([x, y], axis=1), np.stack([x + 7, y], axis=1)


def reference(cur, forw, pair, cfg):
    """The restatement's result with the spread of F under two one-ulp perturbations, computed once per case."""
    key = ("ref", cur.tobytes(), forw.tobytes(), pair, tuple(sorted(cfg.items())))
    if key not in _cache:
        cam = euroc()
        ref = rr.reject(cam, cur, forw, pair, cfg)
        spread = np.zeros((3, 3))
        if ref["status"] == rr.OK and ref["hyp"] >= 0:
            rng = np.random.RandomState(5)
            for _ in range(2):
                p = rr.reject(cam, cur, forw, pair, cfg, perturb=rng)
                if (p["status"], p["hyp"]) == (ref["status"], ref["hyp"]) and np.array_equal(p["mask"], ref["mask"]):
                    spread = np.fmax(spread, np.abs(p["F"] - ref["F"]))
        ref["spread"] = spread
        _cache[key] = ref
    return _cache[key]


def check(got, ref, name):
    assert ref["margin"] >= MIN_MARGIN, (name, ref["margin"])            # the restatement alone must decide every point clearly
    assert (got["status"], got["hyp"], got["n_inliers"]) == (ref["status"], ref["hyp"], ref["n_inliers"]), \
        (name, got["status"], got["hyp"], got["n_inliers"], ref["status"], ref["hyp"], ref["n_inliers"])
    assert got["mask"].dtype == bool and np.array_equal(got["mask"], ref["mask"]), name
    assert np.array_equal(np.isnan(got["F"]), np.isnan(ref["F"])), name
    if not np.isnan(ref["F"]).any():
        bar = 10.0 * float(ref["spread"].max()) + 1e-13 * max(1.0, float(np.abs(ref["F"]).max()))
        err = float(np.abs(got["F"] - ref["F"]).max())
        print("%-24s hyp %4d inliers %4d margin %.2e  F err %.3e bar %.3e" % (name, ref["hyp"], ref["n_inliers"], ref["margin"], err, bar))
        assert err <= bar, (name, err, bar)


def run_case(rh, cur, forw, pair=0, name="", **cfg):
    rh.set_config(**cfg)
    got = rh.reject_batch([dict(cur_pts=cur, forw_pts=forw, pair=pair)])[0]
    ref = reference(cur, forw, pair, cfg)
    check(got, ref, name)
    return got, ref


# (n, scene seed): n = 7 is the size gate, n = 8 draws all eight points in every hypothesis
SHAPES = [(7, 0), (8, 0), (9, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (4096, 0)]


@pytest.mark.parametrize("n,seed", SHAPES)
def test_shapes(rh, n, seed):
    cur, forw = scene(n, seed) if n > 9 else scene(9, seed, outlier_share=0.0)      # (eight points with an outlier among them fit nothing)
    got, ref = run_case(rh, cur[:n], forw[:n], pair=n, name="n=%d" % n)
    if n < 8:
        assert (ref["status"], ref["hyp"]) == (rr.OK, -1) and got["mask"].all() and np.isnan(got["F"]).all()
    else:
        assert ref["status"] == rr.OK and 0 < ref["n_inliers"] <= n


@pytest.mark.parametrize("H", [1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1, 4096])
def test_hypothesis_counts(rh, H):
    cur, forw = scene(150, 1)
    _, ref = run_case(rh, cur, forw, pair=2, name="H=%d" % H, ransac_hypotheses=H)
    # (the one hypothesis of H = 1 draws an outlier and reaches no 8 inliers: the no-model outcome on a scene that has a model)
    assert ref["status"] == (rr.FAIL_NO_MODEL if H == 1 else rr.OK) and 0 <= ref["hyp"] < H


@pytest.mark.parametrize("H,pair", [(ROUND + 1, 352), (2 * ROUND + 1, 298)])
def test_winner_in_the_last_partial_round(rh, H, pair):
    cur, forw = scene(60, 11, noise_px=0.5)
    _, ref = run_case(rh, cur, forw, pair=pair, name="last round H=%d" % H, ransac_hypotheses=H)
    assert ref["status"] == rr.OK and ref["hyp"] == H - 1 and ref["winner_round"] == (H - 1) // ROUND and H % ROUND == 1


@pytest.mark.parametrize("seed,pair", [(0, 0), (0xFFFFFFFF, 0), (0, 2 ** 32 - 1), (0xFFFFFFFF, 2 ** 32 - 1)])
def test_seeds_and_pairs(rh, seed, pair):
    cur, forw = scene(150, 2)
    _, ref = run_case(rh, cur, forw, pair=pair, name="seed %x pair %x" % (seed, pair), seed=seed)
    assert ref["status"] == rr.OK
    other = reference(cur, forw, 7, dict(seed=seed))
    assert other["hyp"] != ref["hyp"] or pair == 7                       # (the pair enters the sampling)


def test_no_model_keeps_every_pair(rh):
    cur, forw = collinear_pair()
    got, ref = run_case(rh, cur, forw, pair=3, name="collinear")
    assert ref["status"] == rr.FAIL_NO_MODEL and got["mask"].all() and got["n_inliers"] == 8 and np.isnan(got["F"]).all()


def test_batch_is_its_single_calls_byte_for_byte(rh):
    sizes = [4096, 0, 7, 8, 150, 257]
    items = []
    for k, n in enumerate(sizes):
        cur, forw = scene(n, 3) if n > 9 else scene(9, 3, outlier_share=0.0)
        items.append(dict(cur_pts=cur[:n].copy(), forw_pts=forw[:n].copy(), pair=k))
    rh.set_config()
    a, b = rh.reject_batch(items), rh.reject_batch(items)
    singles = [rh.reject_batch([it])[0] for it in items]

    def same(x, y):
        return (x["status"], x["hyp"], x["n_inliers"]) == (y["status"], y["hyp"], y["n_inliers"]) and \
            x["mask"].tobytes() == y["mask"].tobytes() and x["F"].tobytes() == y["F"].tobytes()

    for k, n in enumerate(sizes):
        assert len(a[k]["mask"]) == n and same(a[k], b[k]) and same(a[k], singles[k]), (k, n)
        check(a[k], reference(items[k]["cur_pts"], items[k]["forw_pts"], k, {}), "batch[%d] n=%d" % (k, n))
    # a NaN point in one pair: NOT_FINITE there, the others unchanged bit for bit
    bad = [dict(it) for it in items]
    bad[4] = dict(bad[4], forw_pts=bad[4]["forw_pts"].copy())
    bad[4]["forw_pts"][17, 1] = np.nan
    c = rh.reject_batch(bad)
    assert c[4]["status"] == rr.NOT_FINITE and c[4]["hyp"] == -1 and not c[4]["mask"].any() and np.isnan(c[4]["F"]).all()
    for k in (0, 1, 2, 3, 5):
        assert same(c[k], a[k]), k
    assert same(rh.reject_batch(items)[4], a[4])                          # ... and the handle goes on


def test_argument_errors_write_nothing(vio, reject_lib):
    from vio_amd import reject as rj
    cam = euroc()
    fn = reject_lib.fn
    h = reject_lib.create()
    PAT = 0xA5
    cur, forw = scene(150, 3)
    big = np.zeros((4097, 2), dtype=np.float32)

    def raw_batch(items_spec, null_mask=False):
        n_items = len(items_spec)
        arr = (rj.VioRejectItem * n_items)(*[rj.VioRejectItem(n, 0, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data)
                                             for n, a, b in items_spec])
        res = np.full(n_items * 88, PAT, dtype=np.uint8)
        mask = np.full(8192, PAT, dtype=np.uint8)
        st = fn["batch"](h.h, C.c_int32(n_items), C.addressof(arr), res.ctypes.data, None if null_mask else mask.ctypes.data)
        return st, res, mask

    BAD_ARG = -1
    # no camera set
    st, res, mask = raw_batch([(150, cur, forw)])
    assert st == BAD_ARG and "camera" in h.last_error() and np.all(res == PAT) and np.all(mask == PAT)
    un = np.full((150, 2), 7.5, dtype=np.float32)
    vel = un.copy()
    ids = np.arange(150, dtype=np.int64)
    status = (C.c_int32 * 1)(77)
    it = (rj.VioRejectUndistortItem * 1)(rj.VioRejectUndistortItem(150, 0, cur.ctypes.data, ids.ctypes.data, None, None, 0.0, un.ctypes.data, vel.ctypes.data))
    assert fn["undistort_batch"](h.h, C.c_int32(1), C.addressof(it), C.addressof(status)) == BAD_ARG
    assert status[0] == 77 and np.all(un == 7.5) and np.all(vel == 7.5)
    out = np.full((150, 2), 7.5)
    assert fn["lift"](h.h, C.c_int32(150), cur.ctypes.data, out.ctypes.data) == BAD_ARG and np.all(out == 7.5)
    # a model that is not PINHOLE is refused and sets nothing
    with pytest.raises(vio.VioError):
        h.set_camera(**dict(rr.EUROC, model=rj.MODEL_PINHOLE + 1))
    assert raw_batch([(150, cur, forw)])[0] == BAD_ARG
    h.set_camera(**rr.EUROC)
    # n = 4097, in the second item: the first is not computed either
    st, res, mask = raw_batch([(150, cur, forw), (4097, big, big)])
    assert st == BAD_ARG and "item 1" in h.last_error() and np.all(res == PAT) and np.all(mask == PAT)
    # a NULL array
    for spec, nm in (([(150, cur, None)], False), ([(150, None, forw)], False), ([(150, cur, forw)], True)):
        st, res, mask = raw_batch(spec, null_mask=nm)
        assert st == BAD_ARG and np.all(res == PAT) and np.all(mask == PAT)
    assert fn["batch"](h.h, C.c_int32(1), None, None, None) == BAD_ARG and fn["batch"](h.h, C.c_int32(-1), None, None, None) == BAD_ARG
    assert fn["batch"](h.h, C.c_int32(0), None, None, None) == 0          # count == 0 is VIO_OK
    assert fn["undistort_batch"](h.h, C.c_int32(0), None, None) == 0
    # 0 hypotheses: refused, the configuration stays
    for bad_cfg in (dict(ransac_hypotheses=0), dict(ransac_hypotheses=4097), dict(f_threshold=0.0), dict(focal_length=float("nan"))):
        with pytest.raises(vio.VioError):
            h.set_config(**bad_cfg)
    # dt = 0 with m > 0 (and n = 4097, a NULL output)
    prev_un = rr.un_points(cam, cur)
    for n, m, dt, unp in ((150, 150, 0.0, un), (150, 150, float("nan"), un), (150, 150, -1.0, un), (4097, 0, 0.1, un), (150, 4097, 0.1, un), (150, 0, 0.1, None)):
        it = (rj.VioRejectUndistortItem * 1)(rj.VioRejectUndistortItem(n, m, cur.ctypes.data, ids.ctypes.data, ids.ctypes.data, prev_un.ctypes.data, dt,
                                                                       None if unp is None else unp.ctypes.data, vel.ctypes.data))
        assert fn["undistort_batch"](h.h, C.c_int32(1), C.addressof(it), C.addressof(status)) == BAD_ARG, (n, m, dt)
        assert status[0] == 77 and np.all(un == 7.5) and np.all(vel == 7.5)
    assert fn["lift"](h.h, C.c_int32(4097), big.ctypes.data, out.ctypes.data) == BAD_ARG and np.all(out == 7.5)
    assert fn["lift"](h.h, C.c_int32(150), None, out.ctypes.data) == BAD_ARG
    # the handle works on a following valid call, with the configuration it had
    check(h.reject_batch([dict(cur_pts=cur, forw_pts=forw, pair=4)])[0], reference(cur, forw, 4, {}), "after errors")
    got_un, got_vel = h.undistort(cur, ids, ids, prev_un, 0.05)
    assert got_un.tobytes() == prev_un.tobytes() and not got_vel.any()
    h.close()


def test_device_is_restored_and_timing(rh):
    import torch
    cur, forw = scene(150, 3)
    before = torch.cuda.current_device()
    rh.reject(cur, forw, 1)
    t = rh.timing()
    assert torch.cuda.current_device() == before
    assert t["kernel_ms"] > 0 and t["total_ms"] >= t["kernel_ms"]


# ---- the front end -------------------------------------------------------------------------------------------
def test_frontend_with_the_three_handles(vio, rh):
    frames = fixture_frames() + [fixture_frames()[1]]
    fh, dh = vio.load_flow().create(), vio.load_detect().create()

    def run(rejecter):
        ft = vio.FeatureTracker(fh, dh, max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=rejecter)
        outs = []
        for t, img in enumerate(frames):
            o = ft.read_image(img, 0.05 * t)
            o["ids_after"] = ft.update_ids()
            o["ff"] = ft.feature_frame()
            outs.append(o)
        return outs

    rh.set_config()
    a, b = run(rh), run(rr.Rejecter(euroc()))
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("pts", "ids", "track_cnt", "un_pts", "velocity", "ids_after"):
            assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), (t, k)
        assert np.array_equal(x["ff"][0], y["ff"][0]) and x["ff"][1].tobytes() == y["ff"][1].tobytes(), t
    assert len(a[2]["ff"][0]) > 50 and np.any(a[3]["velocity"] != 0)
    check_frames(vio.FeatureTracker(fh, dh, max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=rh), fixture_frames())
    fh.close()
    dh.close()
