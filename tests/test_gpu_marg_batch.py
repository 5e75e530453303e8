"""Batched marginalisation on the GPU (csrc/libvio_marg_hip.so, include/vio_marg.h) against vio_marginalize on a context loaded with
the same arrays, and the batch's own guarantees: bitwise independence of the batch, per-window failure, argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marg_reference as mr  # noqa: E402
import vio_testutil as tu  # noqa: E402
from test_oracle_golden import cfg_of  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOWS = ["window_n50_s42", "window_n300_s43", "window_n300_s45_prior", "window_n200_s46_huber", "window_n200_s46_tukey",
           "window_n120_s44_ragged_extfree", "window_noimu_n300_s48_prior"]


def golden(vio, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return tu.arrays_to_window(vio, z), cfg_of(z)


@pytest.fixture(scope="module")
def marg_lib(vio, hip_lib):
    return vio.load_marg()


def with_prior(vio, hip_lib, w, kw):
    """w with a marginalisation prior of its own (vio_marginalize of the window itself), for the windows that have none."""
    if w.prior is not None:
        return w
    c = hip_lib.context(**kw)
    c.load(w)
    p = c.marginalize(vio.MARG_OLD)
    c.close()
    return vio.synth.Window(**dict(w.__dict__, prior=p)) if hasattr(w, "__dict__") else w._replace(prior=p)


def reference(hip_lib, kind, w, kw):
    c = hip_lib.context(**kw)
    c.load(w)
    out = c.marginalize(kind)
    c.close()
    return out


def check_against(m, ref, Hin, bin_, frame):
    """test_marg_reference.check_against_exact: check_prior's invariants against vio_marginalize's prior, and its two entry-wise bars
    against the Schur complement evaluated in 50-digit arithmetic from the oracle's dense input (or no farther from it than
    vio_marginalize's own prior, whose QL tail misses it by up to 8e-5 on the windows with an IMU edge)."""
    from test_marg_reference import check_against_exact
    check_against_exact(m, ref, Hin, bin_, frame)


def without_huber_ambiguous(vio, oracle_lib, w, kw):
    """w without the landmarks whose Huber weight test is decided by rounding (cov_reference.huber_ambiguous: rho' + 2 rho'' e2 > 0 is
    zero in exact arithmetic beyond delta, and two libraries forming the residual in different orders may decide it differently)."""
    import cov_reference as cr
    c = oracle_lib.context(**kw)
    amb = cr.huber_ambiguous(oracle_lib, c.cfg, w, np.asarray(w.poses), np.asarray(w.ext), np.asarray(w.inv_depth))
    if not amb.any():
        return w
    keep = np.nonzero(~amb)[0]
    new = -np.ones(len(amb), dtype=np.int64)
    new[keep] = np.arange(len(keep))
    e = ~amb[np.asarray(w.lm)]
    return vio.synth.Window(**dict(w.__dict__, inv_depth=np.asarray(w.inv_depth)[keep], lm=new[np.asarray(w.lm)[e]].astype(np.int32),
                                   host=np.asarray(w.host)[e], target=np.asarray(w.target)[e], pts_i=np.asarray(w.pts_i)[e],
                                   pts_j=np.asarray(w.pts_j)[e], n_landmarks=len(keep), n_observations=int(e.sum())))


@pytest.mark.parametrize("kind", [0, 1], ids=["old", "second_new"])
@pytest.mark.parametrize("name", WINDOWS)
def test_single_window_matches_vio_marginalize(vio, hip_lib, oracle_lib, marg_lib, name, kind):
    w, kw = golden(vio, name)
    w = without_huber_ambiguous(vio, oracle_lib, w, kw)
    if kind == vio.MARG_SECOND_NEW:
        w = with_prior(vio, hip_lib, w, kw)
    ref = reference(hip_lib, kind, w, kw)
    got = marg_lib.create(**kw).compute(kind, w, w.prior)
    check_against(got, ref, *oracle_input(oracle_lib, kind, w, kw), 0 if kind == vio.MARG_OLD else vio.WINDOW_SIZE - 1)


def oracle_input(oracle_lib, kind, w, kw):
    c = oracle_lib.context(**kw)
    c.load(w)
    return mr.dense_input(oracle_lib, c, kind)


def test_no_prior_and_no_imu_edge(vio, hip_lib, oracle_lib, marg_lib):
    w, kw = golden(vio, "window_n300_s43")
    w.prior = None
    w.preint = [None] + list(w.preint[1:])
    ref = reference(hip_lib, vio.MARG_OLD, w, kw)
    got = marg_lib.create(**kw).compute(vio.MARG_OLD, w, None)
    check_against(got, ref, *oracle_input(oracle_lib, vio.MARG_OLD, w, kw), 0)


def empty_graph_window(vio, hip_lib):
    """MargOldFrame's smallest graph: no landmark and no observation, IMU edge 0 and a prior (that of make_window(60, seed=21), whose
    states the window keeps)."""
    w = with_prior(vio, hip_lib, vio.synth.make_window(60, seed=21), {})
    z = np.zeros(0, dtype=np.int32)
    return vio.synth.Window(**dict(w.__dict__, inv_depth=np.zeros(0), lm=z, host=z, target=z, pts_i=np.zeros((0, 2)),
                                   pts_j=np.zeros((0, 2)), n_landmarks=0, n_observations=0))


def without_frame0_hosts(vio, w):
    """w without the observations hosted in frame 0, and so without their landmarks (re-indexed as in without_huber_ambiguous):
    MargOldFrame's graph keeps IMU edge 0 and has an empty Schur part."""
    e = np.asarray(w.host) != 0
    keep = np.unique(np.asarray(w.lm)[e])
    new = -np.ones(len(w.inv_depth), dtype=np.int64)
    new[keep] = np.arange(len(keep))
    return vio.synth.Window(**dict(w.__dict__, inv_depth=np.asarray(w.inv_depth)[keep], lm=new[np.asarray(w.lm)[e]].astype(np.int32),
                                   host=np.asarray(w.host)[e], target=np.asarray(w.target)[e], pts_i=np.asarray(w.pts_i)[e],
                                   pts_j=np.asarray(w.pts_j)[e], n_landmarks=len(keep), n_observations=int(e.sum())))


def empty_graph_cases(vio, hip_lib):
    """Both windows carry the prior of make_window(60, seed=21) itself.  Without one MargOldFrame has nothing to compare: frame 0 then
    hangs on IMU edge 0 alone, its 15 x 15 block is invertible, and the exact Schur complement is what the pseudo-inverse's cut
    leaves, 0.44 at most, under an input of 4.0e15, whose rounding (2^-53 of it) is 0.44 as well.  Measured on the CPU for the
    window without frame-0 hosts and without a prior: the oracle's own prior misses the 50-digit Schur complement by 2.6 and the
    restatement's by 1.1, so check_against's eigenvalue comparison (2e-5) would compare two roundings.  With the prior the Schur
    complement is 5.0e4 and the oracle's prior is within 1.2e-4 of it."""
    w = with_prior(vio, hip_lib, vio.synth.make_window(60, seed=21), {})
    assert (np.asarray(w.host) == 0).sum() > 0
    no0 = without_frame0_hosts(vio, w)
    assert 0 < no0.n_landmarks < 60 and not (np.asarray(no0.host) == 0).any() and no0.lm.max() == no0.n_landmarks - 1
    return {"no_landmarks": empty_graph_window(vio, hip_lib), "no_frame0_hosts": no0}


@pytest.mark.parametrize("case", ["no_landmarks", "no_frame0_hosts"])
def test_marg_old_with_an_empty_schur_part(vio, hip_lib, oracle_lib, marg_lib, case):
    """MARG_OLD of a window with n = 0, m = 0 (IMU edge 0 and a prior only) and of one in which no landmark is hosted in frame 0,
    against vio_marginalize on a context loaded with the same arrays (or, should the context refuse a window without landmarks,
    against the restatement's tail on the oracle's dense input), and bitwise the same inside a batch of ordinary windows."""
    w = empty_graph_cases(vio, hip_lib)[case]
    Hin, bin_ = oracle_input(oracle_lib, vio.MARG_OLD, w, {})
    try:
        ref = reference(hip_lib, vio.MARG_OLD, w, {})
    except vio.VioError:
        assert case == "no_landmarks"
        ref = mr.tail(Hin, bin_, 0)[0]
    mh = marg_lib.create()
    got = mh.compute(vio.MARG_OLD, w, w.prior)
    assert all(np.isfinite(got[k]).all() for k in ("H", "b", "err", "jt_inv"))
    print(case, "live rows", mh.live_rows(0), int((np.abs(ref["H"]).sum(1) > 0).sum()))
    assert mh.live_rows(0) == int((np.abs(ref["H"]).sum(1) > 0).sum())
    check_against(got, ref, Hin, bin_, 0)
    jobs = mixed_jobs(vio, hip_lib, 6)
    jobs.insert(1, (vio.MARG_OLD, w, w.prior))
    jobs.insert(5, (vio.MARG_OLD, w, w.prior))
    res = mh.compute_batch(jobs)
    assert same(res[1], got) and same(res[5], got)
    for i in (0, 2, 4, 7):
        assert same(res[i], mh.compute(*jobs[i])), i


def test_reference_kat(vio, hip_lib, marg_lib):
    import test_marg_kat as kat
    w = vio.synth.make_window(8, seed=3)
    out = marg_lib.create().compute(vio.MARG_SECOND_NEW, w, kat.kat_prior())
    kat.check_output(out)


def mixed_jobs(vio, hip_lib, count):
    """count windows: golden and synthetic, both kinds, with and without priors."""
    jobs = []
    rng = np.random.RandomState(5)
    for i in range(count):
        if i % 4 == 0:
            w, _ = golden(vio, WINDOWS[(i // 4) % 4])       # (the default configuration's windows)
        else:
            w = vio.synth.make_window(int(rng.choice([40, 150, 300])), seed=100 + i)
        kind = vio.MARG_SECOND_NEW if i % 5 == 3 else vio.MARG_OLD
        prior = w.prior
        if kind == vio.MARG_SECOND_NEW and prior is None:
            prior = with_prior(vio, hip_lib, w, {}).prior
        if i % 3 == 2:
            prior = None if kind == vio.MARG_OLD else prior
        jobs.append((kind, w, prior))
    return jobs


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("H", "b", "err", "jt_inv"))


def test_batch_of_64_is_bitwise_each_window_alone(vio, hip_lib, marg_lib):
    jobs = mixed_jobs(vio, hip_lib, 64)
    # window 17: a landmark hosted in frame 0 at infinite inverse depth has h_l = 0 exactly: no inverse
    kind, w, prior = jobs[17]
    w = vio.synth.make_window(60, seed=77)
    l0 = int(w.lm[np.nonzero(w.host == 0)[0][0]])
    w.inv_depth = w.inv_depth.copy()
    w.inv_depth[l0] = np.inf
    jobs[17] = (vio.MARG_OLD, w, prior)
    mh = marg_lib.create()
    with pytest.raises(vio.VioError) as ei:
        mh.compute_batch(jobs)
    res = ei.value.results
    st = ei.value.window_status
    assert st[17] == -3 and all(s == 0 for i, s in enumerate(st) if i != 17)
    assert np.all(res[17]["H"] == 0) and np.all(np.isnan(res[17]["b"])) and np.all(np.isnan(res[17]["jt_inv"]))
    again = mh.compute_batch(jobs, allow_nonfinite=True)
    for i in range(64):
        assert same(res[i], again[i]), i
        alone = mh.compute(*jobs[i], allow_nonfinite=True)
        assert same(res[i], alone), i
    assert all(np.isfinite(res[i]["H"]).all() for i in range(64) if i != 17)


def test_all_156_rows_live(vio, marg_lib):
    rng = np.random.RandomState(3)
    A = rng.normal(size=(156, 156))
    H = A @ A.T + 156 * np.eye(156)
    prior = dict(H=H, b=rng.normal(size=156))
    mh = marg_lib.create()
    out = mh.compute(vio.MARG_SECOND_NEW, None, prior)
    assert mh.live_rows(0) == 141          # 156 minus the 15 marginalised
    keep = [i for i in range(156) if not (6 + 15 * 9 <= i < 6 + 15 * 10)]
    mm = [i for i in range(156) if 6 + 15 * 9 <= i < 6 + 15 * 10]
    S = H[np.ix_(keep, keep)] - H[np.ix_(keep, mm)] @ np.linalg.solve(H[np.ix_(mm, mm)], H[np.ix_(mm, keep)])
    # (MargNewFrame moves frame 9 to the end: the kept block keeps its order, frame 10's rows shift up by 15 — the latter are zero here)
    got = out["H"][:141, :141]
    assert np.abs(got - S).max() <= 1e-10 * np.abs(S).max()
    assert np.abs(out["jt_inv"].T @ out["jt_inv"] @ out["H"] - np.eye(156) * (np.abs(out["H"]).sum(1) > 0)).max() <= 1e-8


def test_20000_landmark_window(vio, hip_lib, oracle_lib, marg_lib):
    w = vio.synth.make_window(20000, seed=11)
    ref = reference(hip_lib, vio.MARG_OLD, w, {})
    got = marg_lib.create().compute(vio.MARG_OLD, w, None)
    check_against(got, ref, *oracle_input(oracle_lib, vio.MARG_OLD, w, {}), 0)


def test_batched_prior_solves_like_vio_marginalize_prior(vio, hip_lib, marg_lib):
    w, kw = golden(vio, "window_n300_s45_prior")
    ref = reference(hip_lib, vio.MARG_OLD, w, kw)
    got = marg_lib.create(**kw).compute(vio.MARG_OLD, w, w.prior)
    w2, _ = golden(vio, "window_n300_s43")
    out = []
    for p in (ref, got):
        c = hip_lib.context(**kw)
        w2.prior = p
        c.load(w2)
        rep = c.solve(10)
        poses, sb, ext = c.get_window()
        out.append((rep.final_chi2, poses, sb))
    # (the two priors differ by the Schur complement's rounding, O(1e-5) of H: measured 2e-5 of chi2 on this window)
    assert abs(out[0][0] - out[1][0]) <= 1e-4 * abs(out[0][0])
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-6 * np.abs(out[0][1]).max()
    assert np.abs(out[0][2] - out[1][2]).max() <= 1e-6 * max(np.abs(out[0][2]).max(), 1.0)


def test_run_batched_matches_drivers_alone(vio, hip_lib, marg_lib):
    from vio_amd import batch_stream, stream as vs      # noqa: F401
    seeds = list(range(8))
    first = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=seeds[0]), nonkey_every=0)
    sh = first.ctx.get_stream()
    batched = [first] + [vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=s), ctx_kwargs=dict(stream=sh),
                                         nonkey_every=3 if s % 2 else 0) for s in seeds[1:]]
    trajs = batch_stream.run_batched(batched, marg_lib.create(stream=sh))
    assert any(vio.MARG_SECOND_NEW in d.flags for d in batched) and all(vio.MARG_OLD in d.flags for d in batched)
    for s, d, tr in zip(seeds, batched, trajs):
        alone = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=s), nonkey_every=3 if s % 2 else 0)
        ta = alone.run()
        assert tr.shape == ta.shape
        # (measured up to 5.5e-3 m over 16 frames: the two priors differ by the Schur complement's rounding, and the stream carries
        #  that difference from frame to frame; the accuracy below is what must not change)
        assert np.abs(tr - ta).max() <= 2e-2
        gt = alone.ground_truth()
        ea, eb = vs.ate_rmse(ta, gt), vs.ate_rmse(tr, d.ground_truth())
        assert abs(ea - eb) <= 0.03 * ea           # (measured 1.1 % on one seed of the eight)


def test_run_batched_refuses_unbatched_options(vio, hip_lib, marg_lib):
    from vio_amd import batch_stream, stream as vs
    d = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=12, seed=1), outlier_px=3.0)
    with pytest.raises(ValueError, match="outlier_px"):
        batch_stream.run_batched([d], marg_lib.create())


def test_argument_errors(vio, hip_lib, marg_lib):
    mh = marg_lib.create()
    w = vio.synth.make_window(30, seed=2)
    assert mh.compute_batch([]) == []
    with pytest.raises(vio.VioError) as ei:
        mh.compute(7, w, None)
    assert "window 0" in mh.last_error()
    bad = vio.synth.make_window(30, seed=2)
    bad.target = bad.host.copy()
    with pytest.raises(vio.VioError):
        mh.compute_batch([(vio.MARG_OLD, w, None), (vio.MARG_OLD, bad, None)])
    assert "window 1" in mh.last_error()
    bad2 = vio.synth.make_window(30, seed=2)
    bad2.lm = bad2.lm.copy()
    bad2.lm[0] = 10 ** 6
    with pytest.raises(vio.VioError):
        mh.compute(vio.MARG_OLD, bad2, None)
    with pytest.raises(vio.VioError):
        mh.compute(vio.MARG_OLD, None, None)         # null state arrays
    with pytest.raises(vio.VioError, match="UNSUPPORTED"):
        mh.compute(vio.MARG_OLD, vio.synth.make_window_xyz(30, seed=2), None)
