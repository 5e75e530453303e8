"""libvio_camera_hip on the GPU (include/vio_camera.h) against tests/camera_reference.py and against
libvio_reject_hip: PINHOLE byte for byte the rejection library's; MEI, SCARAMUZZA and a KANNALA_BRANDT camera without coefficients
every bit and every mask of the restatement; KANNALA_BRANDT's theta within the error of the reference's own method, its rays within
C 2^-53 of the 50-digit values, its RANSAC exactly the restatement's on the device's own rays; an item independent of its batch, its
position and its slot's number; the argument rules; the front end through a CameraHandle.

Measured on an MI355X (DESIGN.md section 27 has the table): theta errors of 1.0e-16 to 1.1e-16 against E_ref of 1.8e-15 to 4.7e-15
(0.010 to 0.028 of the bound); ray errors of 1.3 to 1.8 x 2^-53, from which VIO_CAMERA_KB_RAY_C = 3.6; every other comparison exact."""
import ctypes as C
import os
import sys

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_reference as cr  # noqa: E402
import frame_sequences as fs  # noqa: E402
import reject_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
MIN_MARGIN = 1e-6
BAD_ARG = -1
_cache = {}
# slot -> camera: the four models, and two more slots of models already there with other parameters
SLOTS = {0: cr.EUROC, 1: cr.KB_FOUR, 2: cr.MEI, 3: cr.SCARAMUZZA, 4: cr.MEI_XI1, 5: cr.KB_CURVED, 6: cr.KB_ZERO, 7: cr.KB_TWO, 8: cr.MEI_PLAIN}
NS = [0, 1, 63, 64, 65, 255, 256, 257]
MS = [0, 1, 1024, 1025]


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_camera(), vio.load_reject()


@pytest.fixture()
def ch(libs):
    h = libs[1].create()
    for s, p in SLOTS.items():
        h.set_camera(slot=s, **p)
    yield h
    h.close()


def ref_cam(params):
    key = ("cam",) + tuple(sorted(params.items()))
    if key not in _cache:
        _cache[key] = cr.Camera(**params)
    return _cache[key]


def pixels(n, cam, seed=1):
    """n pixels inside the frame and, for a KANNALA_BRANDT camera, inside r(theta_max)."""
    rng = np.random.RandomState(seed + n)
    c, r = cr.centre(cam), 0.95 * cr.field_radius(cam)
    return (c + rng.uniform(-1, 1, (n, 2)) * r / np.sqrt(2.0)).astype(np.float32)


def scene(params, n, seed=1, **kw):
    key = ("scene", n, seed, tuple(sorted(kw.items()))) + tuple(sorted(params.items()))
    if key not in _cache:
        _cache[key] = cr.two_view_scene(ref_cam(params), n=n, seed=seed, **kw)
    return _cache[key]


def und_item(params, slot, n, m, seed):
    cam = ref_cam(params)
    rng = np.random.RandomState(100 * seed + n + m)
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    if n > 2:
        ids[1] = -1
    prev_ids = rng.permutation(max(3 * max(n, m) + 8, 16)).astype(np.int64)[:m]
    prev_un = rng.uniform(-0.5, 0.5, (m, 2)).astype(np.float32)
    return dict(pts=pixels(n, cam, seed), ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un, dt=0.05, slot=slot)


def lift_bytes(o):
    return (o["status"], o["n_clamped"], o["rays"].tobytes(), o["angles"].tobytes())


def und_bytes(o):
    return (o["status"], o["n_clamped"], o["un_pts"].tobytes(), o["velocity"].tobytes())


def rej_bytes(o):
    return (o["status"], o["hyp"], o["n_inliers"], o["mask"].tobytes(), o["F"].tobytes())


# ---- an item is its own: batch, position, slot number, repetition ----------------------------------------------------------
def test_items_do_not_depend_on_batch_position_or_slot(libs, ch):
    order = [0, 1, 2, 3, 4, 5, 6, 7]                                    # item k: slot order[k], n = NS[k], m = MS[k % 4]
    items = [und_item(SLOTS[s], s, NS[k], MS[k % 4], seed=k) for k, s in enumerate(order)]
    a, b = ch.undistort_batch(items), ch.undistort_batch(items)
    la, lb = ch.lift_batch(items), ch.lift_batch(items)
    assert [und_bytes(o) for o in a] == [und_bytes(o) for o in b] and [lift_bytes(o) for o in la] == [lift_bytes(o) for o in lb]
    # alone, and in reverse order
    for k, it in enumerate(items):
        assert und_bytes(ch.undistort_batch([it])[0]) == und_bytes(a[k]), k
        assert lift_bytes(ch.lift_batch([it])[0]) == lift_bytes(la[k]), k
        assert len(a[k]["un_pts"]) == NS[k] and a[k]["status"] == cr.OK
    rev = ch.undistort_batch(items[::-1])[::-1]
    assert [und_bytes(o) for o in rev] == [und_bytes(o) for o in a]
    # the same cameras under other slot numbers, on another handle
    other = libs[1].create()
    try:
        for s, p in SLOTS.items():
            other.set_camera(slot=255 - s, **p)
        moved = [dict(it, slot=255 - it["slot"]) for it in items]
        assert [und_bytes(o) for o in other.undistort_batch(moved)] == [und_bytes(o) for o in a]
        assert [lift_bytes(o) for o in other.lift_batch(moved)] == [lift_bytes(o) for o in la]
        pairs = [dict(cur_pts=scene(SLOTS[s], 40, seed=s)[0], forw_pts=scene(SLOTS[s], 40, seed=s)[1], pair=s, slot=s) for s in (0, 1, 2, 3, 4, 5)]
        r1, r2 = ch.reject_batch(pairs), ch.reject_batch(pairs)
        assert [rej_bytes(o) for o in r1] == [rej_bytes(o) for o in r2]
        for k, it in enumerate(pairs):
            assert rej_bytes(ch.reject_batch([it])[0]) == rej_bytes(r1[k]), k
        assert [rej_bytes(o) for o in other.reject_batch([dict(it, slot=255 - it["slot"]) for it in pairs][::-1])[::-1]] == [rej_bytes(o) for o in r1]
    finally:
        other.close()
    # the id lookup found what the restatement finds (the velocities of the bit-exact models are compared in full below)
    k = 5
    ref = cr.undistort(ref_cam(SLOTS[order[k]]), items[k]["pts"], items[k]["ids"], items[k]["prev_ids"], items[k]["prev_un_pts"], 0.05,
                       rays=la[k]["rays"])
    assert a[k]["velocity"].tobytes() == ref[1].tobytes() and a[k]["un_pts"].tobytes() == ref[0].tobytes()


# ---- PINHOLE is the rejection library's, byte for byte -------------------------------------------------------------------------
def test_pinhole_equals_the_reject_library(libs, ch):
    rh = libs[2].create()
    try:
        rh.set_camera(**rr.EUROC)
        cfg = dict(seed=5, ransac_hypotheses=130, f_threshold=1.0, focal_length=460.0)
        rh.set_config(**cfg)
        ch.set_config(**cfg)
        cam = ref_cam(cr.EUROC)
        for n in NS:
            p = pixels(n, cam, seed=2)
            rays = ch.lift(p, slot=0)
            assert rays[:, :2].tobytes() == rh.lift(p).tobytes() and np.all(rays[:, 2] == 1.0), n
        items = [und_item(cr.EUROC, 0, n, m, seed=9) for n, m in zip(NS, MS + MS)]
        mine, theirs = ch.undistort_batch(items), rh.undistort_batch(items)
        for x, y in zip(mine, theirs):
            assert (x["status"], x["un_pts"].tobytes(), x["velocity"].tobytes()) == (y["status"], y["un_pts"].tobytes(), y["velocity"].tobytes())
        cur, forw = scene(cr.EUROC, 257, seed=4)
        line = np.stack([np.arange(8, dtype=np.float32) * 40 + 100, np.full(8, 200, dtype=np.float32)], axis=1)
        pairs = [dict(cur_pts=cur[:n], forw_pts=forw[:n], pair=n, slot=0) for n in (7, 8, 65, 150, 257)] + \
                [dict(cur_pts=line, forw_pts=line + np.float32([7, 0]), pair=3, slot=0)]
        mine, theirs = ch.reject_batch(pairs), rh.reject_batch(pairs)
        assert [rej_bytes(o) for o in mine] == [rej_bytes(o) for o in theirs]
        assert mine[-1]["status"] == cr.FAIL_NO_MODEL and mine[3]["status"] == cr.OK and 8 <= mine[3]["n_inliers"] < 150
    finally:
        rh.close()


# ---- the models that are arithmetic alone: every bit, every mask -------------------------------------------------------------
BIT_EXACT = [("mei", 2), ("mei_plain", 8), ("mei_xi1", 4), ("scaramuzza", 3), ("kb_zero", 6)]


def check_masks(got, ref, name):
    assert ref["margin"] >= MIN_MARGIN, (name, ref["margin"])            # the restatement alone must decide every point clearly
    assert (got["status"], got["hyp"], got["n_inliers"]) == (ref["status"], ref["hyp"], ref["n_inliers"]), \
        (name, got["status"], got["hyp"], got["n_inliers"], ref["status"], ref["hyp"], ref["n_inliers"])
    assert np.array_equal(got["mask"], ref["mask"]), name


@pytest.mark.parametrize("name,slot", BIT_EXACT)
def test_bit_exact_models(ch, name, slot):
    """Every model here is arithmetic alone on the device: kb_zero's theta is rho, and its atan2, sin and cos are the library's own
    (csrc/vio_camera_math.h), restated operation for operation."""
    params = SLOTS[slot]
    cam = ref_cam(params)
    ch.set_config()
    for n in (1, 257):
        p = pixels(n, cam, seed=3)
        got, ref = ch.lift_batch([dict(pts=p, slot=slot)])[0], cam.lift(p)
        assert got["n_clamped"] == 0 and got["status"] == cr.OK
        assert got["angles"].tobytes() == np.stack([ref["theta"], ref["phi"]], axis=1).tobytes(), (name, n)
        assert got["rays"].tobytes() == ref["rays"].tobytes(), (name, n, float(np.abs(got["rays"] - ref["rays"]).max()))
    it = und_item(params, slot, 257, 1025, seed=4)
    it["prev_ids"][:200] = it["ids"][:200][::-1]
    got = ch.undistort_batch([it])[0]
    un, vel, st = cr.undistort(cam, it["pts"], it["ids"], it["prev_ids"], it["prev_un_pts"], 0.05)
    assert (got["status"], got["un_pts"].tobytes(), got["velocity"].tobytes()) == (st, un.tobytes(), vel.tobytes()) and np.any(vel != 0)
    for n in (8, 150):
        cur, forw = scene(params, 150, seed=6) if n > 9 else scene(params, 9, seed=6, outlier_share=0.0)
        got = ch.reject_batch([dict(cur_pts=cur[:n], forw_pts=forw[:n], pair=n, slot=slot)])[0]
        check_masks(got, cr.reject(cam, cur[:n], forw[:n], pair=n), "%s n=%d" % (name, n))


def test_kb_zero_rays_equal_the_restatement_in_every_bit(ch):
    """KANNALA_BRANDT without coefficients: theta = rho, phi = atan2 and the ray (sin theta cos phi, sin theta sin phi, cos theta), every
    bit of the restatement's.  With the device math library's atan2, sin and cos this did not hold (on an MI355X 63 of 257 phi and 130
    of 771 ray components differed from glibc's in the last bit, at most 3.6e-16): no two math libraries round alike.  The library
    now computes the three in arithmetic of its own, which the device, the host build and the restatement share."""
    cam = ref_cam(cr.KB_ZERO)
    p = np.concatenate([pixels(257, cam, seed=3), cr.centre(cam)[None].astype(np.float32), np.float32([[0, 0], [511, 0], [254, 300], [100, 256.5]])])
    got, ref = ch.lift_batch([dict(pts=p, slot=6)])[0], cam.lift(p)
    assert got["angles"][:, 0].tobytes() == ref["theta"].tobytes()
    diff = got["rays"] != ref["rays"]
    print("kb_zero: %d of %d ray components differ from the restatement's, largest difference %.3e; %d of %d phi differ" %
          (diff.sum(), diff.size, np.abs(got["rays"] - ref["rays"]).max(), (got["angles"][:, 1] != ref["phi"]).sum(), len(p)))
    assert got["angles"][:, 1].tobytes() == ref["phi"].tobytes()
    assert got["rays"].tobytes() == ref["rays"].tobytes()


# ---- KANNALA_BRANDT with coefficients ------------------------------------------------------------------------------------------
KB = [("four", 1), ("two", 7), ("curved", 5)]


def kb_truth(name):
    key = ("kb", name)
    if key not in _cache:
        cam = ref_cam(cr.KB_CAMERAS[name])
        pts, n_out = cr.kb_points(cam)
        keep, exact, e_ref = cr.kb_theta_errors(cam, pts)
        _cache[key] = (cam, pts, n_out, keep, exact, e_ref)
    return _cache[key]


@pytest.mark.parametrize("name,slot", KB)
def test_kannala_brandt_theta_rays_and_clamping(ch, name, slot):
    cam, pts, n_out, keep, exact, e_ref = kb_truth(name)
    got = ch.lift_batch([dict(pts=pts, slot=slot)])[0]
    ref = cam.lift(pts)
    assert got["status"] == cr.OK and got["n_clamped"] == n_out == int(ref["clamped"].sum())
    th, ph, rays = got["angles"][:, 0], got["angles"][:, 1], got["rays"]
    assert np.all(th[ref["clamped"]] == float(cam.theta_max)) and ph[0] == 0.0
    with mpmath.workdps(50):
        err = [abs(mpmath.mpf(float(th[i])) - t) for i, t in zip(keep, exact)]
        worst = max(float(e / mpmath.mpf(cr.theta_bound(e_ref, t))) for e, t in zip(err, exact))
        # the ray at the exact theta and the exact phi of the device's own p_u (phi's inputs are arithmetic alone: the restatement's)
        rho, _ = cam.kb_polar(pts)
        c = cam.pin
        p64 = pts.astype(np.float64)
        px, py = c.ik11 * p64[:, 0] + c.ik13, c.ik22 * p64[:, 1] + c.ik23
        ray_err = 0.0
        for i, t in zip(keep, exact):
            f = mpmath.mpf(0) if rho[i] < 1e-10 else mpmath.atan2(mpmath.mpf(float(py[i])), mpmath.mpf(float(px[i])))
            want = [mpmath.sin(t) * mpmath.cos(f), mpmath.sin(t) * mpmath.sin(f), mpmath.cos(t)]
            ray_err = max(ray_err, max(float(abs(mpmath.mpf(float(rays[i, k])) - want[k])) for k in range(3)))
    print("%s: E_ref %.3e  device theta error %.3e (%.3f of the bound)  ray error %.3f x 2^-53" %
          (name, e_ref, float(max(err)), worst, ray_err * 2.0 ** 53))
    assert worst <= 1.0, (name, worst)
    assert ray_err <= cr.KB_RAY_C * 2.0 ** -53, (name, ray_err * 2.0 ** 53)
    # theta, phi and the rays are arithmetic alone: the restatement's, in every bit
    assert got["angles"].tobytes() == np.stack([ref["theta"], ref["phi"]], axis=1).tobytes() and rays.tobytes() == ref["rays"].tobytes()
    # un_pts within one float32 ulp of the restatement's
    u = ch.undistort_batch([dict(pts=pts, ids=np.full(len(pts), -1), slot=slot)])[0]
    want = cr.un_points(cam, pts)
    assert u["status"] == cr.OK and u["n_clamped"] == n_out
    assert np.all(np.abs(u["un_pts"].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("name,slot", KB)
def test_kannala_brandt_ransac_on_the_devices_own_rays(ch, name, slot):
    """The trigonometry taken out: the restatement fed the device's lift_batch rays must give vio_camera_reject_batch's hyp, n_inliers
    and masks exactly."""
    params = cr.KB_CAMERAS[name]
    cam = ref_cam(params)
    ch.set_config(seed=2)
    cases = []
    for n in (7, 8, 150):
        cur, forw = scene(params, 150, seed=7) if n > 9 else scene(params, 9, seed=7, outlier_share=0.0)
        cases.append((cur[:n], forw[:n], n))
    # eight points that all moved onto one pixel: the second set has no extent, its normalisation divides by zero, F is NaN in every
    # hypothesis and no point is an inlier: no model, on the device and in the restatement alike (NaN goes where NaN goes)
    cases.append((cases[1][0], np.repeat(cases[1][1][:1], 8, axis=0), 3))
    got = ch.reject_batch([dict(cur_pts=a, forw_pts=b, pair=p, slot=slot) for a, b, p in cases])
    lifted = ch.lift_batch([dict(pts=x, slot=slot) for a, b, _ in cases for x in (a, b)])
    for k, (a, b, p) in enumerate(cases):
        ref = cr.reject(cam, a, b, pair=p, cfg=dict(seed=2), rays=(lifted[2 * k]["rays"], lifted[2 * k + 1]["rays"]))
        if k == 3:                                                        # (every error is NaN there: there is no margin to speak of)
            assert ref["status"] == cr.FAIL_NO_MODEL and (got[k]["status"], got[k]["hyp"], got[k]["n_inliers"]) == (ref["status"], ref["hyp"], 8)
        elif len(a) >= 8:
            check_masks(got[k], ref, "%s case %d" % (name, k))
        else:
            assert (got[k]["status"], got[k]["hyp"]) == (cr.OK, -1) and got[k]["mask"].all() and np.isnan(got[k]["F"]).all()
    assert got[3]["status"] == cr.FAIL_NO_MODEL and got[3]["mask"].all() and got[2]["status"] == cr.OK


# ---- rules -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(libs):
    vio = libs[0]
    from vio_amd import camera as cm
    h = libs[1].create()
    fn, PAT = libs[1].fn, 0xA5
    cam = ref_cam(cr.MEI)
    cur, forw = scene(cr.MEI, 150, seed=3)
    ids = np.arange(150, dtype=np.int64)
    big = np.zeros((4097, 2), dtype=np.float32)

    def raw_reject(spec, count=None, null_mask=False):
        arr = (cm.VioCameraRejectItem * len(spec))(*[cm.VioCameraRejectItem(n, 0, None if a is None else a.ctypes.data,
                                                                             None if b is None else b.ctypes.data, s, 0) for n, a, b, s in spec])
        res, mask = np.full(len(spec) * 88, PAT, dtype=np.uint8), np.full(8192, PAT, dtype=np.uint8)
        st = fn["reject_batch"](h.h, C.c_int32(len(spec) if count is None else count), C.addressof(arr), res.ctypes.data,
                                None if null_mask else mask.ctypes.data)
        return st, bool(np.all(res == PAT) and np.all(mask == PAT))

    def raw_points(n, m, slot, dt=0.05, un_null=False, p=cur, lift=True):
        un, vel = np.full((4100, 2), 7.5, dtype=np.float32), np.full((4100, 2), 7.5, dtype=np.float32)
        rays, ang = np.full((4100, 3), 7.5), np.full((4100, 2), 7.5)
        res = (cm.VioCameraLiftResult * 1)(cm.VioCameraLiftResult(77, 77))
        it = (cm.VioCameraUndistortItem * 1)(cm.VioCameraUndistortItem(n, m, p.ctypes.data, ids.ctypes.data, ids.ctypes.data, cur.ctypes.data, dt,
                                                                        None if un_null else un.ctypes.data, vel.ctypes.data, slot, 0))
        st_u = fn["undistort_batch"](h.h, C.c_int32(1), C.addressof(it), C.addressof(res))
        li = (cm.VioCameraLiftItem * 1)(cm.VioCameraLiftItem(n, slot, p.ctypes.data, None if un_null else rays.ctypes.data, ang.ctypes.data))
        st_l = fn["lift_batch"](h.h, C.c_int32(1), C.addressof(li), C.addressof(res)) if lift else BAD_ARG
        clean = res[0].status == 77 and res[0].n_clamped == 77 and np.all(un == 7.5) and np.all(vel == 7.5) and np.all(rays == 7.5) and np.all(ang == 7.5)
        return st_u, st_l, bool(clean)

    # an unset slot (nothing is set yet), a slot out of range
    for slot in (0, 255, 256, -1):
        assert raw_reject([(150, cur, forw, slot)]) == (BAD_ARG, True) and "slot" in h.last_error()
        assert raw_points(150, 0, slot) == (BAD_ARG, BAD_ARG, True)
    # cameras that are refused set nothing
    refused = [dict(cr.KB_FOUR, k2=-0.9), dict(cr.KB_FOUR, mu=0.0), dict(cr.MEI, gamma2=0.0), dict(cr.EUROC, fx=0.0),
               dict(cr.KB_FOUR, theta_max=3.5), dict(cr.SCARAMUZZA, ac=0.0, ad=0.0), dict(cr.MEI, width=0), dict(cr.MEI, xi=float("inf"))]
    for p in refused:
        with pytest.raises(vio.VioError):
            h.set_camera(slot=0, **p)
        assert raw_reject([(150, cur, forw, 0)]) == (BAD_ARG, True)
    for model in (4, -1):                                                 # an unknown model (the binding would refuse it before the library)
        m = cm.VioCameraModel(model, 752, 480, 0, (C.c_double * 16)(*([1.0] * 16)))
        assert fn["set"](h.h, C.c_int32(0), C.byref(m)) == BAD_ARG and "model" in h.last_error()
    assert fn["set"](h.h, C.c_int32(0), None) == BAD_ARG and raw_reject([(150, cur, forw, 0)]) == (BAD_ARG, True)
    with pytest.raises(vio.VioError):
        h.set_camera(slot=256, **cr.MEI)
    with pytest.raises(vio.VioError):
        h.set_camera(slot=0, **dict(cr.KB_FOUR, k2=-0.9))
    assert "increase" in h.last_error()
    h.set_camera(slot=0, **cr.MEI)
    with pytest.raises(vio.VioError):
        h.set_camera(slot=0, **dict(cr.KB_FOUR, k2=-0.9))               # ... and a refused camera leaves the slot as it was
    # a bad item behind a good one: the first is not computed either
    assert raw_reject([(150, cur, forw, 0), (4097, big, big, 0)]) == (BAD_ARG, True) and "item 1" in h.last_error()
    assert raw_reject([(150, cur, forw, 0), (150, cur, forw, 1)]) == (BAD_ARG, True) and "item 1" in h.last_error()
    # NULL arrays, count out of range
    assert raw_reject([(150, cur, None, 0)]) == (BAD_ARG, True) and raw_reject([(150, None, forw, 0)]) == (BAD_ARG, True)
    assert raw_reject([(150, cur, forw, 0)], null_mask=True) == (BAD_ARG, True)
    assert raw_reject([(150, cur, forw, 0)], count=-1) == (BAD_ARG, True) and raw_reject([(150, cur, forw, 0)], count=4097) == (BAD_ARG, True)
    for name in ("lift_batch", "undistort_batch"):
        assert fn[name](h.h, C.c_int32(1), None, None) == BAD_ARG and fn[name](h.h, C.c_int32(-1), None, None) == BAD_ARG
        assert fn[name](h.h, C.c_int32(4097), None, None) == BAD_ARG and fn[name](h.h, C.c_int32(0), None, None) == 0
    assert fn["reject_batch"](h.h, C.c_int32(1), None, None, None) == BAD_ARG and fn["reject_batch"](h.h, C.c_int32(0), None, None, None) == 0
    assert raw_points(4097, 0, 0, p=big) == (BAD_ARG, BAD_ARG, True)
    assert raw_points(150, 0, 0, un_null=True) == (BAD_ARG, BAD_ARG, True)
    for n, m, dt in ((150, 150, 0.0), (150, 150, float("nan")), (150, 150, -1.0), (150, 4097, 0.05)):
        assert raw_points(n, m, 0, dt=dt, lift=False)[::2] == (BAD_ARG, True), (n, m, dt)    # (m and dt are the undistort call's)
    for bad_cfg in (dict(ransac_hypotheses=0), dict(ransac_hypotheses=4097), dict(f_threshold=0.0), dict(focal_length=float("nan"))):
        with pytest.raises(vio.VioError):
            h.set_config(**bad_cfg)
    # the handle works on a following valid call, with the camera and the configuration it had
    check_masks(h.reject_batch([dict(cur_pts=cur, forw_pts=forw, pair=4)])[0], cr.reject(cam, cur, forw, pair=4), "after errors")
    h.close()


def test_not_finite_items_stand_alone(ch):
    import torch
    before = torch.cuda.current_device()
    ch.set_config()
    h = ch
    h.set_camera(slot=9, model=cr.MODEL_MEI, width=512, height=512, xi=1.0, gamma1=128.0, gamma2=128.0, u0=256.0, v0=256.0)
    cur, forw = scene(cr.MEI, 150, seed=3)
    good = dict(cur_pts=cur, forw_pts=forw, pair=1, slot=2)
    nan = dict(good, forw_pts=forw.copy())
    nan["forw_pts"][17, 1] = np.nan
    flat = np.array([[300.0 + 3 * k, 256.0 + 2 * (k % 5)] for k in range(20)], dtype=np.float32)
    zero = flat.copy()
    zero[11] = [384.0, 256.0]                                           # mx = 1, my = 0: z = (1 - 1) / 2 = 0
    alone = h.reject_batch([good])[0]
    out = h.reject_batch([good, nan, dict(cur_pts=zero, forw_pts=flat, pair=2, slot=9), dict(cur_pts=flat, forw_pts=zero, pair=2, slot=9),
                          dict(cur_pts=zero[8:15], forw_pts=flat[8:15], pair=2, slot=9), good])
    assert rej_bytes(out[0]) == rej_bytes(alone) == rej_bytes(out[5]) and alone["status"] == cr.OK
    for o in out[1:4]:
        assert o["status"] == cr.NOT_FINITE and o["hyp"] == -1 and o["n_inliers"] == 0 and not o["mask"].any() and np.isnan(o["F"]).all()
    assert out[4]["status"] == cr.OK and out[4]["mask"].all()           # n = 7: the size gate comes before the lift
    ids = np.full(20, -1, dtype=np.int64)
    u_alone = h.undistort_batch([dict(pts=cur, ids=np.arange(150), slot=2)])[0]
    u = h.undistort_batch([dict(pts=cur, ids=np.arange(150), slot=2), dict(pts=zero, ids=ids, slot=9), dict(pts=nan["forw_pts"], ids=np.arange(150), slot=2),
                           dict(pts=flat, ids=ids, slot=9)])
    assert und_bytes(u[0]) == und_bytes(u_alone) and u[0]["status"] == cr.OK and u[3]["status"] == cr.OK and np.isfinite(u[3]["un_pts"]).all()
    for o in u[1:3]:
        assert o["status"] == cr.NOT_FINITE and np.isnan(o["un_pts"]).all() and np.isnan(o["velocity"]).all()
    l = h.lift_batch([dict(pts=zero, slot=9), dict(pts=nan["forw_pts"], slot=2)])
    assert l[0]["status"] == cr.OK and l[0]["rays"][11].tolist() == [1.0, 0.0, 0.0] and l[1]["status"] == cr.NOT_FINITE
    t = h.timing()
    assert torch.cuda.current_device() == before and t["kernel_ms"] > 0 and t["total_ms"] >= t["kernel_ms"]


# ---- the front end -------------------------------------------------------------------------------------------------------------
def test_front_end_through_a_camera_handle(libs):
    vio, clib, rlib = libs
    imgs = [fs.image(64, 48, 5, t) for t in range(5)]
    fr, rh, ch = vio.load_frame().create(), rlib.create(), clib.create()
    try:
        fr.set_config(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow=dict(levels=2, half_patch=2), detect=dict(min_distance=3))
        rh.set_camera(**rr.EUROC)
        ch.set_camera(slot=0, **cr.EUROC)
        small_mei = dict(model=cr.MODEL_MEI, width=64, height=48, xi=0.9, k1=-0.05, k2=0.01, p1=1e-4, p2=-1e-4, gamma1=70.0, gamma2=69.0, u0=31.5, v0=23.6)
        ch.set_camera(slot=3, **small_mei)

        def run(rejecter, slot):
            ft = vio.FeatureTracker(None, None, max_cnt=24, min_dist=3, rejecter=rejecter, frames=fr, slot=slot)
            outs = []
            for t, img in enumerate(imgs):
                o = ft.read_image(img, 0.05 * t)
                ft.update_ids()
                o["ff"] = ft.feature_frame()
                outs.append(o)
            return outs

        a, b = run(rh, 0), run(ch, 1)
        for t, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x["ff"][0], y["ff"][0]) and x["ff"][1].dtype == y["ff"][1].dtype and x["ff"][1].tobytes() == y["ff"][1].tobytes(), t
            for k in ("pts", "ids", "track_cnt", "un_pts", "velocity"):
                assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), (t, k)
        assert len(a[-1]["ff"][0]) >= 8 and np.any(a[-1]["velocity"] != 0)
        m = run(ch.bind(3), 2)
        first = next((t for t, (x, y) in enumerate(zip(a, m)) if len(x["ids"]) != len(y["ids"]) or not np.array_equal(x["ids"], y["ids"])), len(imgs))
        for t, (x, y) in enumerate(zip(a, m)):
            if t < first:
                assert np.array_equal(x["ids"], y["ids"]) and x["pts"].tobytes() == y["pts"].tobytes(), t
            ids, rows = y["ff"]
            assert ids.dtype == np.int64 and rows.dtype == np.float64 and rows.shape == (len(ids), 7) and np.isfinite(rows).all(), t
            assert y["un_pts"].dtype == np.float32 and y["un_pts"].shape == (len(y["pts"]), 2) and np.isfinite(y["un_pts"]).all()
            assert y["velocity"].shape == (len(y["pts"]), 2) and np.isfinite(y["velocity"]).all()
    finally:
        for h in (fr, rh, ch):
            h.close()
