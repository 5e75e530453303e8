"""The residual query on the GPU (csrc/libvio_res_hip.so, include/vio_residuals.h) against the numpy reference of
tests/res_reference.py, evaluated on the HIP context's own states; test_residuals_reference.py pins that reference to the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import res_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu


check, rel_err = rr.check, rr.rel_err         # (shared with test_gpu_residuals_limits.py)


@pytest.mark.parametrize("case", rr.CASES, ids=[c[0] for c in rr.CASES])
def test_residuals_match_the_reference(vio, hip_lib, oracle_lib, case):
    w, kw = rr.make_case(vio, oracle_lib, case)
    c = hip_lib.context(**kw)
    c.load(w)
    c.solve(10)
    got = c.residuals(w)
    check(vio, oracle_lib, c, w, got)
    assert got["obs"].shape == (len(w.lm), 4) and got["flags"].dtype == np.uint8


def test_after_a_stepwise_update(vio, hip_lib, oracle_lib):
    """vio_update_states leaves the trial state in the context: the query reads that one, as vio_chi2 does."""
    for case in (rr.CASES[2], rr.CASES[6]):
        w, kw = rr.make_case(vio, oracle_lib, case)
        c = hip_lib.context(**kw)
        c.load(w)
        c.linearize()
        _, lam = c.init_lm()
        c.solve_linear(lam)
        c.update_states()
        check(vio, oracle_lib, c, w, c.residuals(w))


def test_bench_window_20000(vio, hip_lib, oracle_lib):
    """bench.py's window size, with a marginalisation prior."""
    wp = vio.synth.make_window(300, seed=41, t0=0.9)
    cp = oracle_lib.context()
    cp.load(wp)
    cp.solve(5)
    w = vio.synth.make_window(20000, seed=1)
    w.prior = cp.marginalize(vio.MARG_OLD)
    c = hip_lib.context()
    c.load(w)
    c.solve(10)
    got = c.residuals(w)
    check(vio, oracle_lib, c, w, got)
    t = c._res.timing()
    assert all(np.isfinite(v) and v >= 0 for v in t.values()), t


def test_repeated_calls_are_bitwise_identical(vio, hip_lib, oracle_lib):
    for case in (rr.CASES[3], rr.CASES[5], rr.CASES[6]):
        w, kw = rr.make_case(vio, oracle_lib, case)
        c = hip_lib.context(**kw)
        c.load(w)
        c.solve(5)
        a, b = c.residuals(w), c.residuals(w)
        for k in ("obs", "lm", "flags"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        for k, v in a["summary"].items():
            assert np.array_equal(np.asarray(v), np.asarray(b["summary"][k])), k


def test_outputs_may_be_null(vio, hip_lib, oracle_lib):
    w, kw = rr.make_case(vio, oracle_lib, rr.CASES[2])
    c = hip_lib.context(**kw)
    c.load(w)
    c.solve(5)
    full = c.residuals(w)
    h = c._res
    only = h.compute(w, outputs=("summary",))
    assert only["obs"] is None and only["flags"] is None
    assert all(np.array_equal(np.asarray(v), np.asarray(full["summary"][k])) for k, v in only["summary"].items())
    flags = h.compute(w, outputs=("flags",))
    assert np.array_equal(flags["flags"], full["flags"]) and flags["summary"] is None
    noimu = h.compute(w, imu=False)
    assert np.isnan(noimu["summary"]["chi2"]) and np.all(np.isnan(noimu["summary"]["imu_edge"]))
    assert noimu["summary"]["visual_robust"] == full["summary"]["visual_robust"]


def run_stream(vio, hip_lib, with_query):
    """Three frames of solve -> (residual query) -> marginalise -> next frame; what every frame leaves behind."""
    c = hip_lib.context()
    prior, out = None, []
    for k in range(3):
        w = vio.synth.make_window(400, seed=20 + k, t0=1.0 + 0.1 * k)
        w.prior = prior
        c.load(w)
        rep = c.solve(5)
        if with_query:
            c.residuals(w)
        poses, sb, ext = c.get_window()
        rec = [poses, sb, ext, c.get_landmarks(), np.array([rep.iterations, rep.trials, rep.accepted, rep.stop_reason]),
               np.array([rep.initial_chi2, rep.final_chi2, rep.final_lambda]), np.array(rep.chi2_trace), np.array(rep.lambda_trace)]
        prior = c.marginalize(vio.MARG_OLD)
        rec += [prior[x] for x in ("H", "b", "err", "jt_inv")]
        out.append(rec)
    c.close()
    return out


def test_the_query_changes_nothing(vio, hip_lib):
    a, b = run_stream(vio, hip_lib, False), run_stream(vio, hip_lib, True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y, equal_nan=True)


def test_sharded_context_is_refused(vio, hip_lib):
    c = hip_lib.context(shard_rank=0, shard_count=2)
    with pytest.raises(vio.VioError) as ei:
        vio.load_res().create(c)
    assert ei.value.status == -5


def test_bad_arguments_write_nothing(vio, hip_lib):
    w = vio.synth.make_window(50, seed=8)
    c = hip_lib.context()
    c.load(w)
    c.solve(3)
    c.residuals(w)                                     # (the handle exists from here on)
    h = c._res
    n, m = w.n_landmarks, len(w.lm)

    def filled():
        return {"obs": np.full((m, 4), 7.0), "lm": np.full((n, 3), 7.0), "flags": np.full(n, 7, dtype=np.uint8)}

    def untouched(o):
        return np.all(o["obs"] == 7.0) and np.all(o["lm"] == 7.0) and np.all(o["flags"] == 7)

    bad = w.copy()
    bad.lm = np.array(w.lm, dtype=np.int32)
    bad.lm[5] = n                                       # a landmark index out of range
    o = filled()
    with pytest.raises(vio.VioError) as ei:
        h.compute(bad, out=o)
    assert ei.value.status == -1 and untouched(o)
    bad = w.copy()
    bad.target = np.array(w.target, dtype=np.int32)
    bad.target[0] = 11                                  # a frame index out of range
    o = filled()
    with pytest.raises(vio.VioError) as ei:
        h.compute(bad, out=o)
    assert ei.value.status == -1 and untouched(o)
    o = filled()
    o["lm"], o["flags"] = np.full((n + 1, 3), 7.0), np.full(n + 1, 7, dtype=np.uint8)
    with pytest.raises(vio.VioError) as ei:
        h.compute(w, n=n + 1, out=o)                    # not the context's landmark count
    assert ei.value.status == -1 and "landmark count" in str(ei.value)
    assert untouched(o)
    o = filled()
    with pytest.raises(vio.VioError) as ei:
        h.compute(w, focal=0.0, out=o)
    assert ei.value.status == -1 and untouched(o)


def _hip_runtime():
    """The HIP runtime libvio_hip.so runs on (already mapped into this process), not whichever copy the loader would find first."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert paths, "libamdhip64 is not loaded"
    return C.CDLL(paths[0])


def test_current_device_is_restored(vio, hip_lib):
    hip = _hip_runtime()
    count, dev = C.c_int(), C.c_int()
    assert hip.hipGetDeviceCount(C.byref(count)) == 0
    w = vio.synth.make_window(40, seed=2)
    c = hip_lib.context(device=0)
    c.load(w)
    c.solve(2)
    other = 1 if count.value > 1 else 0
    assert hip.hipSetDevice(other) == 0
    try:
        c.residuals(w)
        assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value == other
    finally:
        hip.hipSetDevice(0)


def test_seeded_outliers_are_flagged(vio, hip_lib, oracle_lib):
    w, truth = rr.outlier_window(vio)
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(10)
    got = c.residuals(w, outlier_px=3.0)
    _, lmo, flags, _ = check(vio, oracle_lib, c, w, got)
    near = np.abs(lmo[:, 0] - 3.0) <= 1e-9 * 3.0
    assert np.array_equal(got["flags"][~near] & 1, flags[~near] & 1)
    recall, precision = rr.recall_precision(got["flags"], truth)
    assert recall >= rr.RECALL_MIN and precision >= rr.PRECISION_MIN, (recall, precision)


def _corrupted_stream(vio, fraction=0.08, seed=9):
    st = vio.stream.SyntheticStream(n_frames=24, landmarks_per_frame=25, seed=3)
    rng = np.random.RandomState(seed)
    n = len(st.lm_host)
    bad = set(int(l) for l in rng.choice(n, int(fraction * n), replace=False))
    for l in bad:
        for f in st.lm_obs[l]:
            a = rng.uniform(0, 2 * np.pi)
            st.lm_obs[l][f] = st.lm_obs[l][f] + rng.uniform(15.0, 30.0) / vio.synth.FOCAL * np.array([np.cos(a), np.sin(a)])
    return st, bad


def test_stream_without_a_threshold_is_unchanged(vio, hip_lib):
    a = vio.stream.StreamDriver(hip_lib, vio.stream.SyntheticStream(n_frames=18, landmarks_per_frame=25, seed=3))
    b = vio.stream.StreamDriver(hip_lib, vio.stream.SyntheticStream(n_frames=18, landmarks_per_frame=25, seed=3), outlier_px=None)
    ta, tb = a.run(), b.run()
    assert np.array_equal(ta, tb)
    assert b.rejected == [] and [r.final_chi2 for r in a.reports] == [r.final_chi2 for r in b.reports]


def test_stream_rejects_corrupted_tracks(vio, hip_lib):
    class Seen(vio.stream.StreamDriver):
        def window_arrays(self):
            w, ids = super().window_arrays()
            self.seen = getattr(self, "seen", set()) | set(ids)
            return w, ids

    st, bad = _corrupted_stream(vio)
    keep = Seen(hip_lib, st)
    traj_keep = keep.run()
    st, _ = _corrupted_stream(vio)
    drop = Seen(hip_lib, st, outlier_px=3.0)
    traj_drop = drop.run()
    gt = drop.ground_truth()
    rejected = set(drop.rejected_ids)
    assert len(drop.rejected) == len(drop.reports) and sum(drop.rejected) == len(drop.rejected_ids) == len(rejected)
    assert not rejected & set(drop.tracks)
    solved_bad = bad & drop.seen
    recall = len(rejected & solved_bad) / max(1, len(solved_bad))
    precision = len(rejected & bad) / max(1, len(rejected))
    ate_keep, ate_drop = vio.stream.ate_rmse(traj_keep, gt), vio.stream.ate_rmse(traj_drop, gt)
    print("stream rejection: %d corrupted tracks solved, %d rejected (recall %.3f, precision %.3f); ATE %.5f m kept, %.5f m rejected"
          % (len(solved_bad), len(rejected), recall, precision, ate_keep, ate_drop))
    assert len(solved_bad) > 0 and recall >= 0.5 and precision >= 0.5, (recall, precision)
    assert np.isfinite(ate_keep) and np.isfinite(ate_drop)
