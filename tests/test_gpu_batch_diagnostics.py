"""Batched covariance and residual queries (vio_cov_compute_batch, vio_res_compute_batch).

Every window of a batch runs the single-window kernels' code on its own data, so every output must equal the single call on the same
context bit for bit: pose_cov, landmark variances / covariances, landmark information, pivot ratio, per-edge residuals, landmark
statistics and flags, and every summary field."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

GAUGE_NAMES = ["none", "fix_oldest"]


def topped_up(c, w, prior=None, anchor=False):
    """w with a prior made well-posed from its own H_pp_schur (cov_reference.well_posed_prior), loaded into c."""
    w.prior = prior
    c.load(w)
    c.linearize()
    S0, _ = c.get_schur_system()
    w.prior = cr.well_posed_prior(np.diag(S0), prior, anchor=anchor)
    c.load(w)
    return w


def rank_deficient(vio, n=120, seed=9):
    """Frame 10 without observations and without its IMU edge: its rows of H_pp_schur are zero (the pose factorisation fails)."""
    w = vio.synth.make_window(n, seed=seed)
    keep = (w.host != 10) & (w.target != 10)
    for k in ("lm", "host", "target", "pts_i", "pts_j"):
        setattr(w, k, getattr(w, k)[keep])
    w.preint = list(w.preint)
    w.preint[9] = None
    return w


def batch_of(hip_lib, specs):
    """Contexts on one stream, one per (window, config overrides); each loaded with its window."""
    ctxs = []
    for w, kw in specs:
        c = hip_lib.context(**kw) if not ctxs else hip_lib.context(stream=ctxs[0].get_stream(), **kw)
        c.load(w)
        ctxs.append(c)
    return ctxs


def mixed_inverse_depth(vio, hip_lib, oracle_lib, count, big=False, anchor=False):
    """`count` inverse-depth windows: the cases of cov_reference (Huber, ext_fixed, marginalisation priors), windows without a
    marginalisation prior, a 20 000-landmark one when big, and ragged landmark counts."""
    cases = [c for c in cr.CASES if not c[7]]
    specs = []
    for i in range(count):
        if big and i == count // 2:
            w = vio.synth.make_window(20000, seed=1)
            specs.append((w, {}))
            continue
        case = cases[i % len(cases)]
        if i < len(cases):
            # (gauge 0 in the case anchors frame 0 in the topped-up prior: what a batch queried under gauge "none" needs)
            w, kw, _ = cr.make_case(vio, oracle_lib, case[:6] + (0 if anchor else 1,) + case[7:])
        else:
            w = vio.synth.make_window(60 + 37 * i, seed=100 + i, ragged=bool(i & 1), t0=1.0 + 0.01 * i)
            kw = dict(ext_fixed=i & 1, loss_type=1 + (i % 2))
            if kw["loss_type"] == 1:
                kw["loss_delta"] = 5.0
        specs.append((w, kw))
    ctxs = batch_of(hip_lib, specs)
    # windows not made by make_case get a prior topped up from their own system (a window with a marginalisation prior keeps it)
    for (w, kw), c in zip(specs, ctxs):
        if w.prior is None:
            topped_up(c, w, anchor=anchor)
    return ctxs, [w for w, _ in specs]


def xyz_batch(vio, hip_lib, oracle_lib, anchor=False):
    specs = []
    for case in [c for c in cr.CASES if c[7]]:
        w, kw, _ = cr.make_case(vio, oracle_lib, case[:6] + (0 if anchor else 1,) + case[7:])
        specs.append((w, kw))
    w = vio.synth.make_window_xyz(150, seed=12, t0=1.05)
    specs.append((w, dict(loss_type=2)))
    ctxs = batch_of(hip_lib, specs)
    topped_up(ctxs[-1], w, anchor=anchor)
    return ctxs, [w for w, _ in specs]


def cov_state(c, xyz):
    return c._cov.landmark_information(xyz), c._cov.pivot_ratio()


def assert_cov_equal(vio, hip_lib, ctxs, ws, gauge, xyz):
    got = hip_lib.batch_covariance(ctxs, ws, gauge=gauge)
    states = [cov_state(c, xyz) for c in ctxs]
    for i, (c, w) in enumerate(zip(ctxs, ws)):
        P, L = c.covariance(w, gauge=gauge)
        info, ratio = cov_state(c, xyz)
        assert np.array_equal(got[i][0], P), "window %d pose_cov" % i
        assert np.array_equal(got[i][1], L), "window %d landmarks" % i
        assert np.array_equal(states[i][0], info), "window %d landmark information" % i
        assert states[i][1] == ratio, "window %d pivot ratio" % i
    return got


def assert_res_equal(hip_lib, ctxs, ws, outlier_px=3.0):
    got = hip_lib.batch_residuals(ctxs, ws, outlier_px=outlier_px)
    for i, (c, w) in enumerate(zip(ctxs, ws)):
        r = c.residuals(w, outlier_px=outlier_px)
        for k in ("obs", "lm", "flags"):
            assert np.array_equal(got[i][k], r[k], equal_nan=True), "window %d %s" % (i, k)
        for k, v in r["summary"].items():
            assert np.array_equal(np.asarray(got[i]["summary"][k]), np.asarray(v), equal_nan=True), "window %d summary %s" % (i, k)
    return got


@pytest.mark.parametrize("gauge", GAUGE_NAMES)
@pytest.mark.parametrize("count", [1, 3])
def test_inverse_depth_batch_equals_single_calls(vio, hip_lib, oracle_lib, count, gauge):
    ctxs, ws = mixed_inverse_depth(vio, hip_lib, oracle_lib, count, anchor=(gauge == "none"))
    hip_lib.batch_solve(ctxs, 5)
    assert_cov_equal(vio, hip_lib, ctxs, ws, gauge, False)
    assert_res_equal(hip_lib, ctxs, ws)


def test_sixteen_windows_with_a_20000_landmark_one(vio, hip_lib, oracle_lib):
    ctxs, ws = mixed_inverse_depth(vio, hip_lib, oracle_lib, 16, big=True)
    assert max(w.n_landmarks for w in ws) == 20000
    hip_lib.batch_solve(ctxs, 5)
    got = assert_cov_equal(vio, hip_lib, ctxs, ws, "fix_oldest", False)
    assert all(np.all(L > 0) for _, L in got)
    assert_res_equal(hip_lib, ctxs, ws)
    assert_res_equal(hip_lib, ctxs, ws, outlier_px=0.5)          # (flags set on many landmarks)
    t = ctxs[5]._cov.timing()
    assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
    t = ctxs[5]._res.timing()
    assert all(np.isfinite(v) and v >= 0 for v in t.values()), t


@pytest.mark.parametrize("gauge", GAUGE_NAMES)
def test_xyz_batch_equals_single_calls(vio, hip_lib, oracle_lib, gauge):
    ctxs, ws = xyz_batch(vio, hip_lib, oracle_lib, anchor=(gauge == "none"))
    hip_lib.batch_solve(ctxs, 5)
    assert_cov_equal(vio, hip_lib, ctxs, ws, gauge, True)
    assert_res_equal(hip_lib, ctxs, ws)


def test_window_without_imu_edges_in_a_batch(vio, hip_lib):
    """Residuals of a window without IMU edges equal its single call; its covariance fails in the batch as it fails alone."""
    w0 = vio.synth.make_window(200, seed=31)
    w1 = vio.synth.make_window(150, seed=32)
    w1.preint = [None] * vio.WINDOW_SIZE
    w2 = vio.synth.make_window(180, seed=33, ragged=True)
    ctxs = batch_of(hip_lib, [(w0, {}), (w1, {}), (w2, {})])
    topped_up(ctxs[0], w0)
    topped_up(ctxs[2], w2)
    hip_lib.batch_solve(ctxs, 5)
    ws = [w0, w1, w2]
    got = assert_res_equal(hip_lib, ctxs, ws)
    assert got[1]["summary"]["imu"] == 0.0 and np.all(got[1]["summary"]["imu_edge"] == 0.0)
    with pytest.raises(vio.VioError) as ei:
        hip_lib.batch_covariance(ctxs, ws)
    assert ei.value.window_status[1] == -3 and ei.value.window_status[0] == 0 and ei.value.window_status[2] == 0
    with pytest.raises(vio.VioError) as e1:
        ctxs[1].covariance(w1)
    assert e1.value.status == -3
    for i in (0, 2):
        P, L = ctxs[i].covariance(ws[i])
        assert np.array_equal(ei.value.results[i][0], P) and np.array_equal(ei.value.results[i][1], L)


def test_failing_window_is_isolated(vio, hip_lib, oracle_lib):
    """A rank-deficient window in the middle of a batch: its status and message, its outputs untouched, the others as alone."""
    ctxs, ws = mixed_inverse_depth(vio, hip_lib, oracle_lib, 5)
    hip_lib.batch_solve(ctxs, 5)
    bad = rank_deficient(vio)             # (loaded, not solved: the batch query linearises it first)
    ws.insert(2, bad)
    ctxs.insert(2, hip_lib.context(stream=ctxs[0].get_stream()))
    ctxs[2].load(bad)
    outs = [(np.full((cr.PD, cr.PD), 7.0), np.full(c.n, 7.0)) for c in ctxs]
    with pytest.raises(vio.VioError) as ei:
        vio.load_cov().compute_batch(ctxs, ws, "fix_oldest", out=outs)
    e = ei.value
    assert e.status == -3
    assert e.window_status == [0, 0, -3, 0, 0, 0], e.window_status
    msg = ctxs[2]._cov.lib.fn["last_error"](ctxs[2]._cov.h).decode()
    assert "not positive and finite" in msg and ("pose" in msg or "speed-bias" in msg), msg
    assert "window 2" in str(e)
    assert np.all(outs[2][0] == 7.0) and np.all(outs[2][1] == 7.0)
    assert e.results[2] is None
    for i, (c, w) in enumerate(zip(ctxs, ws)):
        if i == 2:
            with pytest.raises(vio.VioError) as e1:
                c.covariance(w)
            assert e1.value.status == -3 and msg in str(e1.value)
            continue
        P, L = c.covariance(w)
        assert np.array_equal(outs[i][0], P) and np.array_equal(outs[i][1], L)
        assert e.results[i][0] is outs[i][0]
    assert_res_equal(hip_lib, ctxs, ws)


def _sentinels(ctxs):
    return [(np.full((cr.PD, cr.PD), 7.0), np.full(c.n, 7.0)) for c in ctxs]


def _res_sentinels(ctxs, ws):
    return [{"obs": np.full((w.lm.size, 4), 7.0), "lm": np.full((c.n, 3), 7.0), "flags": np.full(c.n, 7, dtype=np.uint8)}
            for c, w in zip(ctxs, ws)]


def _untouched(covs, ress):
    return all(np.all(P == 7.0) and np.all(L == 7.0) for P, L in covs) and \
        all(np.all(o["obs"] == 7.0) and np.all(o["lm"] == 7.0) and np.all(o["flags"] == 7) for o in ress)


def test_argument_errors_write_nothing(vio, hip_lib):
    cov, res = vio.load_cov(), vio.load_res()
    w0, w1 = vio.synth.make_window(80, seed=51), vio.synth.make_window(90, seed=52)
    # contexts on different streams
    a, b = hip_lib.context(), hip_lib.context()
    a.load(w0)
    b.load(w1)
    assert a.get_stream() != b.get_stream()
    for ctxs, ws in (([a, b], [w0, w1]),):
        covs, ress = _sentinels(ctxs), _res_sentinels(ctxs, ws)
        with pytest.raises(vio.VioError) as ei:
            cov.compute_batch(ctxs, ws, out=covs)
        assert ei.value.status == -1 and "stream" in str(ei.value)
        with pytest.raises(vio.VioError) as ei:
            res.compute_batch(ctxs, ws, out=ress)
        assert ei.value.status == -1 and "stream" in str(ei.value)
        assert _untouched(covs, ress)
    # one kind of landmark per batch
    wx = vio.synth.make_window_xyz(70, seed=53)
    c = hip_lib.context(stream=a.get_stream())
    c.load(wx)
    for ctxs, ws in (([a, c], [w0, wx]), ([c, a], [wx, w0])):
        covs, ress = _sentinels(ctxs), _res_sentinels(ctxs, ws)
        covs[ws.index(wx)] = (covs[ws.index(wx)][0], np.full((wx.n_landmarks, 3, 3), 7.0))
        with pytest.raises(vio.VioError) as ei:
            cov.compute_batch(ctxs, ws, out=covs)
        assert ei.value.status == -1 and "window 1" in str(ei.value)
        with pytest.raises(vio.VioError) as ei:
            res.compute_batch(ctxs, ws, out=ress)
        assert ei.value.status == -1 and "window 1" in str(ei.value)
        assert _untouched(covs, ress)
    # the same context twice (one handle holds one window)
    covs = _sentinels([a, a])
    with pytest.raises(vio.VioError) as ei:
        cov.compute_batch([a, a], [w0, w0], out=covs)
    assert ei.value.status == -1 and _untouched(covs, [])
    # a sharded context
    s = hip_lib.context(shard_rank=0, shard_count=2, stream=a.get_stream())
    with pytest.raises(vio.VioError) as ei:
        hip_lib.batch_covariance([a, s], [w0, w1])
    assert ei.value.status == -5
    with pytest.raises(vio.VioError) as ei:
        hip_lib.batch_residuals([a, s], [w0, w1])
    assert ei.value.status == -5
    # an empty batch is a no-op
    assert hip_lib.batch_covariance([], []) == [] and hip_lib.batch_residuals([], []) == []
    assert cov.fn["compute_batch"](None, 0, 1, 0, None, None) == 0
    assert res.fn["compute_batch"](None, 0, 0, None, 1.0, 3.0) == 0
    assert cov.fn["compute_batch"](None, -1, 1, 0, None, None) == -1


def run_batch_stream(vio, hip_lib, oracle_lib, with_queries):
    """Three frames of batch solve -> (batch queries) -> marginalise -> next frame, on three windows; what each frame leaves."""
    ctxs = None
    priors = [None, None, None]
    out = []
    for k in range(3):
        ws = [vio.synth.make_window(150 + 50 * j, seed=60 + 10 * j + k, t0=1.0 + 0.1 * k) for j in range(3)]
        for w, p in zip(ws, priors):
            w.prior = p
        if ctxs is None:
            ctxs = batch_of(hip_lib, [(w, {}) for w in ws])
        else:
            for c, w in zip(ctxs, ws):
                c.load(w)
        hip_lib.batch_solve(ctxs, 5)
        if with_queries:
            try:
                hip_lib.batch_covariance(ctxs, ws)
            except vio.VioError as e:         # (windows without a prior may be singular; the states must not care either way)
                assert e.status == -3
            hip_lib.batch_residuals(ctxs, ws)
        rec = []
        for j, c in enumerate(ctxs):
            poses, sb, ext = c.get_window()
            rec += [poses, sb, ext, c.get_landmarks(), np.array([c.chi2()])]
            priors[j] = c.marginalize(vio.MARG_OLD)
            rec += [priors[j][x] for x in ("H", "b", "err", "jt_inv")]
        out.append(rec)
    for c in ctxs:
        c.close()
    return out


def test_batch_queries_change_nothing(vio, hip_lib, oracle_lib):
    a = run_batch_stream(vio, hip_lib, oracle_lib, False)
    b = run_batch_stream(vio, hip_lib, oracle_lib, True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y, equal_nan=True)


def test_two_batch_calls_are_bitwise_identical(vio, hip_lib, oracle_lib):
    ctxs, ws = mixed_inverse_depth(vio, hip_lib, oracle_lib, 4)
    hip_lib.batch_solve(ctxs, 5)
    c1, c2 = hip_lib.batch_covariance(ctxs, ws), hip_lib.batch_covariance(ctxs, ws)
    r1, r2 = hip_lib.batch_residuals(ctxs, ws), hip_lib.batch_residuals(ctxs, ws)
    for x, y in zip(c1, c2):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    for x, y in zip(r1, r2):
        for k in ("obs", "lm", "flags"):
            assert np.array_equal(x[k], y[k], equal_nan=True)
        for k in x["summary"]:
            assert np.array_equal(np.asarray(x["summary"][k]), np.asarray(y["summary"][k]), equal_nan=True)
