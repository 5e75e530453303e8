"""Marginalisation on the GPU where it is well-conditioned, and at its limits: vio_marg_compute_batch (k_marg_build, k_marg_tail) and
vio_marginalize (vio_kernels.hip, host tail) against the Schur complement in 50-digit arithmetic.

The windows of test_gpu_marg_batch.py carry an IMU edge of information 4e15 (cond(Amm) ~1e11), so the bars there are 2e-5 of max|H|.
Here the IMU edge is soft or absent (marg_reference.soft_imu, limit_cases), every fp64 implementation sits within a few 1e-14 of the
exact value, and the device is held to marg_reference.tight_check: 10 x the host references' own distance (the restatement's tail and
the oracle's prior of the same dense input, computed in the test) + 1e-13, relative to max|S| and max(|b|, 1).  No bar is a constant
tuned to the device.  test_marg_reference.py holds the references themselves to 1e-12 on the same windows, on the CPU.

Measured on one MI355X, relative to max|S| (H) and max(|b|, 1) (b); the bars were 1.0e-13 .. 5.5e-13, the references themselves
1.0e-15 .. 4.5e-14 away:
  family                                        batched H / b          vio_marginalize H / b
  no IMU edge, 4 losses (66 rows)               3.7e-14 / 3.7e-14      5.5e-14 / 7.0e-14
  soft IMU 1e-4, 1e-2, 1, gravity (75 rows)     4.4e-14 / 3.7e-14      6.3e-14 / 7.4e-14
  hosted0 1, 255, 256, 257, 513                 2.5e-14 / 5.2e-14      1.9e-14 / 4.6e-14
  ragged 300 and its second stage               3.2e-14 / 3.1e-14      1.6e-14 / 5.9e-14
  soft IMU + dense prior, MARG_OLD (147 rows)   4.5e-14 / 4.2e-14      3.8e-14 / 8.2e-14
  MARG_SECOND_NEW of the dense prior (141)      2.6e-14 / 2.9e-16      2.2e-15 / 1.8e-16
The factor stays 10.  P = jt_inv^T jt_inv on the windows with an empty band: within 0.3 x the bar at most (soft IMU at scale 1).

Besides: the live-row edges (0, 33, 66, 75, 147 rows), the packer's bitwise rules, the five ways into the non-finite outcome, the
argument errors through the raw entry point, and vio_marg_set_config.
Huber: an edge beyond delta has rho' + 2 rho'' e2 = 0 exactly and its weight is decided by rounding, so landmarks
with such an edge are dropped (cov_reference.huber_ambiguous).  On the outlier window with delta = 1 that is every landmark (the case is
a third nothing-live window); the case with delta = 10 keeps 15."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marg_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("H", "b", "err", "jt_inv")
# the contexts of libvio_hip may refuse a window without landmarks; every other window must go through vio_marginalize too
CONTEXT_MAY_REFUSE = {"noimu_huber1_halfinfo"}


@pytest.fixture(scope="module")
def marg_lib(vio, hip_lib):
    return vio.load_marg()


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def by_context(vio, hip_lib, kind, w, kw, may_refuse=False):
    """vio_marginalize on a context loaded with w, or None where the context refuses the window (an argument error, not a failure)."""
    c = hip_lib.context(**kw)
    try:
        c.load(w)
        return c.marginalize(kind)
    except vio.VioError as e:
        if not (may_refuse and e.status in (-1, -4, -5)):
            raise
        print("vio_marginalize refuses the window:", e)
        return None
    finally:
        c.close()


def hold(vio, hip_lib, oracle_lib, marg_lib, name, kind, w, kw, spectrum_expected, may_refuse=False):
    """Both libraries on (kind, w, kw) held to tight_check and spectrum_check; the batched library's prior and the distances."""
    Hin, bin_, rest, orc = mr.references(oracle_lib, kind, w, kw)
    frame = mr.frame_of(kind)
    mh = marg_lib.create(**kw)
    got = mh.compute(kind, w, w.prior)
    assert mh.live_rows(0) == len(mr.live_set(rest["H"]))
    mh.close()
    out = {"batched": got}
    ctx = by_context(vio, hip_lib, kind, w, kw, may_refuse)
    if ctx is not None:
        out["vio_marginalize"] = ctx
    dist = {}
    for label, m in out.items():
        dist[label] = mr.tight_check(m, Hin, bin_, frame, [rest, orc], name=name + " " + label)
        assert mr.spectrum_check(m, Hin, bin_, frame, orc, name + " " + label) == spectrum_expected
    return got, dist, (Hin, bin_, rest, orc)


@pytest.mark.parametrize("name", mr.LIMIT_NAMES)
def test_tight_accuracy(vio, hip_lib, oracle_lib, marg_lib, name):
    kind, w, kw, amb = mr.limit_case(name)
    if amb:
        w = mr.drop_huber_ambiguous(oracle_lib, w, kw)
    got, dist, refs = hold(vio, hip_lib, oracle_lib, marg_lib, name, kind, w, kw, name in mr.SPECTRUM_CASES, name in CONTEXT_MAY_REFUSE)
    assert name in CONTEXT_MAY_REFUSE or "vio_marginalize" in dist
    if name in mr.EXPECT_LIVE:
        assert dist["batched"]["live"] == mr.EXPECT_LIVE[name]
    if name == "soft_1e-4_gravity":
        # gravity reaches the kernel: it moves b by far more than the bar
        k0, w0, kw0, _ = mr.limit_case("soft_1e-4")
        base = marg_lib.create(**kw0).compute(k0, w0, None)
        assert np.abs(base["b"] - got["b"]).max() >= 1e6 * dist["batched"]["bar_b"]
    if name == "second_new_dense_prior":
        # |err|^2 = b^T S^-1 b: every one of the 141 eigenvalues is far above the cut (cond(S) ~ 10: the fp64 solve is good to 1e-14)
        Hin, bin_, rest, _ = refs
        live = mr.live_set(rest["H"])
        S, bs = mr.exact_schur(Hin, bin_, mr.frame_of(kind), live)
        assert np.linalg.cond(S) < 1e3
        want = float(bs @ np.linalg.solve(S, bs))
        for m in (got, by_context(vio, hip_lib, kind, w, kw)):
            assert abs(float(m["err"] @ m["err"]) - want) <= 1e-10 * want


def test_second_stage_on_the_devices_own_prior(vio, hip_lib, oracle_lib, marg_lib):
    """ragged300's prior as the batched library computed it, fed back as the prior of the next window: the window's prior is set before
    the reference contexts are loaded, so the references see the device's prior as their input."""
    kind, w, kw, _ = mr.limit_case("ragged300")
    first = marg_lib.create(**kw).compute(kind, w, None)
    w2 = mr.second_stage(first)
    Hin, bin_, _, _ = mr.references(oracle_lib, vio.MARG_OLD, w2, {})
    applies = mr.band_is_empty(mr.tail_full(Hin, bin_, 0)[3])
    print("second stage: the band around the cut is empty:", applies)
    hold(vio, hip_lib, oracle_lib, marg_lib, "second stage", vio.MARG_OLD, w2, {}, applies)


# ---- live-row edges --------------------------------------------------------------------------------------
def ordinary_jobs(vio):
    return [(vio.MARG_OLD, mr.soft_window(1e-2), None), (vio.MARG_SECOND_NEW, None, mr.dense_spd_prior(1e3)),
            (vio.MARG_OLD, mr.packer_window(), None)]


@pytest.mark.parametrize("case", ["marg_old", "second_new"])
def test_nothing_live(vio, oracle_lib, marg_lib, case):
    if case == "marg_old":
        job = (vio.MARG_OLD, mr.nothing_live_window(), None)
    else:
        job = (vio.MARG_SECOND_NEW, vio.synth.make_window(8, seed=3), mr.frame9_only_prior())
    mh = marg_lib.create()
    got = mh.compute(*job)
    assert mh.live_rows(0) == 0
    assert all(not got[k].any() for k in KEYS)
    jobs = ordinary_jobs(vio)
    alone = [mh.compute(*j) for j in jobs]
    batch = [jobs[0], job, jobs[1], jobs[2], job]
    res = mh.compute_batch(batch)
    assert mh.window_status == [0] * 5
    assert [mh.live_rows(i) for i in (0, 1, 2, 4)] == [75, 0, 141, 0] and mh.live_rows(3) > 0
    assert same(res[1], got) and same(res[4], got)
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert same(res[i], alone[j]), i
        assert np.abs(res[i]["H"]).max() > 0


# ---- bitwise properties of the packer ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["interleaved", "only_frame0", "unobserved", "nan_outside"])
def test_packer_rules_are_bitwise(vio, marg_lib, variant):
    w = mr.packer_window()
    v = {"interleaved": mr.interleaved, "only_frame0": mr.only_frame0, "unobserved": mr.with_unobserved_landmark,
         "nan_outside": mr.nan_outside_graph}[variant](w)
    mh = marg_lib.create()
    base = mh.compute(vio.MARG_OLD, w, None)
    assert np.isfinite(base["H"]).all() and mh.live_rows(0) > 0
    got = mh.compute(vio.MARG_OLD, v, None)           # (status OK: compute raises otherwise)
    assert same(got, base)


def test_h_prior_is_read_through_its_lower_triangle(vio, marg_lib):
    """include/vio_marg.h: H_prior is taken as symmetric and read through its lower triangle, as Eigen's SelfAdjointEigenSolver reads
    the reduced system in problem.cc:766, so a NaN above the diagonal is never read."""
    w, p = mr.soft_window(1e-2), mr.dense_spd_prior(1e3)
    mh = marg_lib.create()
    base = mh.compute(vio.MARG_OLD, w, p)
    q = dict(p, H=p["H"].copy())
    q["H"][40, 97] = np.nan
    assert same(mh.compute(vio.MARG_OLD, w, q), base) and np.isfinite(base["H"]).all()


# ---- non-finite outcomes -----------------------------------------------------------------------------------
def nonfinite_case(vio, trigger):
    """(config overrides, the affected job, three ordinary neighbours)"""
    kw = {}
    if trigger == "tukey3":
        w, kw = mr.tukey3_window()
        job = (vio.MARG_OLD, w, None)
    elif trigger in ("inv_depth_0", "nan_pts_j"):
        w = mr.soft_window(1e-2)
        e0 = int(np.nonzero(np.asarray(w.host) == 0)[0][5])
        if trigger == "inv_depth_0":
            w.inv_depth = np.array(w.inv_depth)
            w.inv_depth[int(w.lm[e0])] = 0.0
        else:
            w.pts_j = np.array(w.pts_j)
            w.pts_j[e0, 1] = np.nan
        job = (vio.MARG_OLD, w, None)
    else:
        p = mr.dense_spd_prior(1e3)
        if trigger == "nan_H_prior":
            p["H"][97, 40] = np.nan           # (the lower triangle: the one H_prior is read through)
        else:
            p["b"][12] = np.nan
        job = (vio.MARG_OLD, mr.soft_window(1e-2), p)
    near = [(vio.MARG_OLD, mr.quiet_window(30, 1), None), (vio.MARG_SECOND_NEW, None, mr.dense_spd_prior(1e3)),
            (vio.MARG_OLD, mr.soft_imu(mr.quiet_window(30, 3), 16, 1e-2), mr.dense_spd_prior(1.0))]
    return kw, job, near


@pytest.mark.parametrize("trigger", ["tukey3", "inv_depth_0", "nan_pts_j", "nan_H_prior", "nan_b_prior"])
def test_nonfinite_outcome(vio, marg_lib, trigger):
    kw, job, near = nonfinite_case(vio, trigger)
    mh = marg_lib.create(**kw)
    alone = [mh.compute(*j) for j in near]
    assert all(np.isfinite(a[k]).all() for a in alone for k in KEYS)
    with pytest.raises(vio.VioError) as ei:
        mh.compute_batch([near[0], job, near[1], near[2]])
    assert ei.value.status == -3 and ei.value.window_status == [0, -3, 0, 0]
    assert "window 1" in mh.last_error()
    res = ei.value.results
    assert not res[1]["H"].any() and all(np.isnan(res[1][k]).all() for k in ("b", "err", "jt_inv"))
    assert mh.live_rows(1) == 0
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert same(res[i], alone[j]), i
    one = mh.compute(*job, allow_nonfinite=True)
    assert same(one, res[1])


# ---- argument errors through the raw entry point --------------------------------------------------------------
SENTINEL = 7.25


def raw_items(vio, mh, jobs, keep):
    """The items of `jobs` as the Python binding fills them, their output arrays filled with SENTINEL."""
    items = (vio.marg.VioMargItem * len(jobs))()
    outs = []
    for i, j in enumerate(jobs):
        it, out = mh._item(*j, keep)
        for k in KEYS:
            out[k][...] = SENTINEL
        items[i] = it
        outs.append(out)
    return items, outs


ARG_ERRORS = ["frame_11", "frame_minus_1", "two_in_one_frame", "two_hosts", "two_pts_i", "H_prior_alone", "null_output", "n_minus_1"]


@pytest.mark.parametrize("error", ARG_ERRORS)
def test_argument_error_in_the_last_window_writes_nothing(vio, marg_lib, error):
    mh = marg_lib.create()
    w = mr.packer_window()
    bad = w.copy()
    prior = None
    if error in ("frame_11", "frame_minus_1"):
        bad.target = np.array(w.target)
        bad.target[7] = 11 if error == "frame_11" else -1
    elif error == "two_in_one_frame":
        bad.target = np.array(w.target)
        assert w.lm[0] == w.lm[1]
        bad.target[1] = bad.target[0]
    elif error == "two_hosts":
        bad.host = np.array(w.host)
        assert w.lm[0] == w.lm[1] and w.target[1] != 8
        bad.host[1] = 8
    elif error == "two_pts_i":
        bad.pts_i = np.array(w.pts_i)
        bad.pts_i[1, 1] += 1e-9
    elif error == "H_prior_alone":
        prior = mr.dense_spd_prior(1.0)
    keep = []
    items, outs = raw_items(vio, mh, [(vio.MARG_OLD, w, None), (vio.MARG_SECOND_NEW, None, mr.dense_spd_prior(1.0)), (vio.MARG_OLD, bad, prior)], keep)
    if error == "H_prior_alone":
        items[2].b_prior = None
    elif error == "null_output":
        items[2].err = None
    elif error == "n_minus_1":
        items[2].n = -1
    ws = (C.c_int32 * 3)(55, 55, 55)
    st = mh.lib.fn["compute_batch"](mh.h, C.c_int32(3), C.cast(items, C.c_void_p), C.cast(ws, C.c_void_p))
    assert st == -1
    assert "window 2" in mh.last_error(), mh.last_error()
    for out in outs:
        assert all((out[k] == SENTINEL).all() for k in KEYS)
    assert list(ws) == [55, 55, 55]
    # the handle still works, and the first two windows were in order
    good = mh.compute_batch([(vio.MARG_OLD, w, None), (vio.MARG_SECOND_NEW, None, mr.dense_spd_prior(1.0))])
    assert all(np.isfinite(g["H"]).all() and g["H"].any() for g in good)


def test_count_and_items_are_checked(vio, marg_lib):
    mh = marg_lib.create()
    keep = []
    items, outs = raw_items(vio, mh, [(vio.MARG_SECOND_NEW, None, mr.dense_spd_prior(1.0))], keep)
    ws = (C.c_int32 * 1)(55)
    fn = mh.lib.fn["compute_batch"]
    assert fn(mh.h, C.c_int32(-1), C.cast(items, C.c_void_p), C.cast(ws, C.c_void_p)) == -1
    assert fn(mh.h, C.c_int32(1), None, C.cast(ws, C.c_void_p)) == -1
    assert all((outs[0][k] == SENTINEL).all() for k in KEYS) and ws[0] == 55
    assert fn(mh.h, C.c_int32(1), C.cast(items, C.c_void_p), C.cast(ws, C.c_void_p)) == 0 and ws[0] == 0
    assert np.isfinite(outs[0]["H"]).all() and (outs[0]["H"] != SENTINEL).any()


# ---- configuration ---------------------------------------------------------------------------------------------
def test_set_config(vio, hip_lib, marg_lib):
    w = mr.soft_window(1e-2)
    other = dict(loss_type=vio.LOSS_HUBER, loss_delta=0.5, reproj_sqrt_info=200.0, gravity=(0.3, -0.2, 9.6))
    used = marg_lib.create()
    first = used.compute(vio.MARG_OLD, w, None)
    fresh = marg_lib.create(**other).compute(vio.MARG_OLD, w, None)
    assert not np.array_equal(first["H"], fresh["H"]) and not np.array_equal(first["b"], fresh["b"])
    default = marg_lib.create().cfg
    used.set_config(marg_lib.create(**other).cfg)
    assert same(used.compute(vio.MARG_OLD, w, None), fresh)
    # a config naming another stream is refused and changes nothing
    ctx = hip_lib.context()
    foreign = marg_lib.create().cfg
    foreign.stream = ctx.get_stream()
    assert foreign.stream
    with pytest.raises(vio.VioError) as ei:
        used.set_config(foreign)
    assert ei.value.status == -1
    assert same(used.compute(vio.MARG_OLD, w, None), fresh)
    used.set_config(default)
    assert same(used.compute(vio.MARG_OLD, w, None), first)
    ctx.close()
