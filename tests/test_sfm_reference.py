"""The numpy restatement of the structure-from-motion (tests/sfm_reference.py) against the ground truth of the synthetic streams.

With pixel noise 0 the recovered rotations, translations and points must equal the ground truth expressed in camera frame l and
scaled to |T[F-1]| = 1.  The bar is 10x the restatement's own error on these two windows, measured once (max-abs over the window):
                                                       rotations (matrix entries)   translations   points
  SyntheticStream(landmarks_per_frame=30, track_len=10)        1.1e-10                1.3e-10      1.0e-9
  RealImuStream(mh05, landmarks_per_frame=40, track_len=10)    2.6e-9                 6.4e-8       1.6e-6
(MH_05's first window starts near rest: 38 px of parallax against 231 px, so its depths are two to three orders worse conditioned.)
Candidate 0 has 30 correspondences at 231 px (synthetic) and 40 at 38.4 px (MH_05), so l = 0 in both.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_reference as sr  # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PX = 1.0 / 460.0
BARS = {"syn": (1.1e-9, 1.3e-9, 1.0e-8), "mh": (2.6e-8, 6.4e-7, 1.6e-5)}


def make_stream(vio, which, noise):
    from vio_amd import stream as vs
    if which == "syn":
        return vs.SyntheticStream(landmarks_per_frame=30, track_len=10, pixel_noise=noise)
    return vs.RealImuStream(dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz"))), landmarks_per_frame=40, track_len=10,
                            pixel_noise=noise)


@pytest.mark.parametrize("which", ["syn", "mh"])
def test_noise_free_window_recovers_the_ground_truth(vio, which):
    st = make_stream(vio, which, 0.0)
    frames = list(range(11))
    item, ids = sr.window_item(st, frames)
    out = sr.sfm(item)
    rel = out["rel"]
    assert out["status"] == sr.OK and rel["l"] == 0
    assert rel["corres"][0] == (30 if which == "syn" else 40)
    assert abs(rel["parallax"][0] - (231.3 if which == "syn" else 38.4)) < 0.1
    assert rel["n_inliers"] == rel["corres"][0] == rel["front"]
    R, T, X, _ = sr.ground_truth(st, frames, rel["l"], ids)
    assert abs(np.linalg.norm(out["T"][-1]) - 1.0) < 1e-12 and np.all(out["T"][0] == 0)
    eR = max(np.abs(sr.quat_to_rot(out["Q"][i]) - R[i]).max() for i in range(11))
    eT = np.abs(out["T"] - T).max()
    m = out["state"]
    assert m.sum() == int((np.diff(item["obs_offset"]) >= 2).sum())        # (the newest frame's own tracks have one observation)
    eX = np.abs(out["points"][m] - X[m]).max()
    print("%s: rotations %.2e translations %.2e points %.2e" % (which, eR, eT, eX))
    bR, bT, bX = BARS[which]
    assert eR <= bR and eT <= bT and eX <= bX, (eR, eT, eX)


@pytest.mark.parametrize("which", ["syn", "mh"])
def test_noisy_window_succeeds_and_the_cost_goes_down(vio, which):
    st = make_stream(vio, which, 0.1 * PX)
    item, _ = sr.window_item(st, list(range(11)))
    out = sr.sfm(item)
    assert out["rel"]["status"] == sr.OK and out["rel"]["l"] == 0 and out["rel"]["front"] > 12
    assert out["status"] == sr.OK and out["fail_frame"] == -1
    assert np.all(out["pnp_iterations"][1:10] >= 1) and out["ba_iterations"] >= 1
    assert out["final_cost"] < out["initial_cost"]


def test_default_track_length_picks_frame_5(vio):
    from vio_amd import stream as vs
    item, _ = sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=5, pixel_noise=0.0), list(range(11)))
    rel = sr.relative_pose(item)
    assert rel["status"] == sr.OK and rel["l"] == 5 and rel["corres"][5] == 30 and np.all(rel["corres"][:5] == 0)
    assert abs(rel["parallax"][5] - 139.0) < 1.0


def test_too_few_correspondences(vio):
    from vio_amd import stream as vs
    item, _ = sr.window_item(vs.SyntheticStream(landmarks_per_frame=15, track_len=1, pixel_noise=0.0), list(range(11)))
    out = sr.sfm(item)
    assert out["status"] == sr.FAIL_RELATIVE_POSE and out["rel"]["l"] == -1 and out["fail_frame"] == -1
    assert out["rel"]["corres"].max() == 15 and np.all(np.isnan(out["Q"]))


def test_parallax_under_the_gate(vio):
    """Every candidate has enough correspondences, none 30 px of parallax: the points of the newest frame are the older frame's
    moved by 10 px."""
    rng = np.random.RandomState(0)
    F, n = 6, 40
    base = rng.uniform(-0.4, 0.4, (n, 2))
    pts = np.concatenate([base[:, None, :] + k * 2.0 * PX * np.array([1.0, 0.0]) for k in range(F)], axis=1).reshape(-1, 2)
    item = dict(n_frames=F, start_frame=np.zeros(n, dtype=np.int32), obs_offset=np.arange(n + 1, dtype=np.int64) * F, pts=pts)
    rel = sr.relative_pose(item)
    assert rel["status"] == sr.FAIL_RELATIVE_POSE and rel["l"] == -1
    assert np.all(rel["corres"] == n) and rel["parallax"].max() < 30.0 and abs(rel["parallax"][0] - 10.0) < 1e-9


def test_pnp_with_fewer_than_ten_points_fails_with_its_frame(vio):
    import test_gpu_sfm as tg
    item = tg.sparse_frame_item(vio)
    rel = sr.relative_pose(item)
    assert rel["status"] == sr.OK and rel["l"] == 5
    out = sr.construct(item, rel["l"], rel["R"], rel["T"])
    assert out["status"] == sr.FAIL_PNP and out["fail_frame"] == 4 and np.all(np.isnan(out["T"]))


def test_inner_track_fixtures_reach_the_last_step_of_construct(vio):
    """The two GPU fixtures with tracks that touch neither frame l nor the newest frame: construct triangulates those from their first
    and last observation (initial_sfm.cpp:196-210), a step none of the plain stream windows reaches (all their tracks with two
    observations are seen in l or in F-1)."""
    import test_gpu_sfm as tg
    ws = dict(tg.windows(vio))
    for name, l, least in (("syn_inner", 0, 30), ("syn_l5_inner", 5, 30)):
        out = sr.sfm(ws[name])
        assert out["status"] == sr.OK and out["rel"]["l"] == l and out["n_remaining"] >= least, (name, out["n_remaining"])
        item = ws[name]
        n = np.diff(item["obs_offset"])
        inner = (n >= 2) & ((item["start_frame"] > l) | (item["start_frame"] + n - 1 < l)) & (item["start_frame"] + n - 1 < 10)
        assert out["n_remaining"] <= inner.sum() and out["state"].sum() == (n >= 2).sum()
    for name in ("syn", "mh_noisy", "syn_l5", "syn_F16"):
        assert sr.sfm(ws[name])["n_remaining"] == 0


def test_not_finite_window():
    item = dict(n_frames=3, start_frame=np.zeros(1, dtype=np.int32), obs_offset=np.array([0, 3]), pts=np.array([[0, 0], [np.nan, 0], [0, 0.1]]))
    assert sr.sfm(item)["status"] == sr.NOT_FINITE


def test_sampling_gives_distinct_indices_below_n():
    """Every n = 8 .. 1000 with every hypothesis h of the default count (candidate n % 11, seed 0), and n = 8 with every h up to
    VIO_SFM_MAX_HYPOTHESES, where the 8 indices must be a permutation.  (The golden list below is written by this restatement, so it
    pins the hash against change; the kernel's copy of the hash is held by the exact hypothesis / mask comparison of
    test_gpu_sfm.py.)"""
    for n in range(8, 1001):
        for h in range(sr.DEFAULT_CFG["ransac_hypotheses"]):
            idx = sr.sample8(0, n % 11, h, n)
            assert len(set(idx)) == 8 and min(idx) >= 0 and max(idx) < n, (n, h, idx)
    for h in range(4096):
        idx = sr.sample8(99, 3, h, 8)
        assert sorted(idx) == list(range(8))


def test_sampling_matches_the_golden_list():
    z = np.load(os.path.join(GOLDEN_DIR, "sfm_sampling.npz"))
    for (seed, i, h, n), idx, h0 in zip(z["keys"], z["indices"], z["hashes"]):
        assert sr.sample8(int(seed), int(i), int(h), int(n)) == list(idx)
        assert sr.hash4(int(seed), int(i), int(h), 0) == int(h0)


def test_jacobi_agrees_with_lapack():
    rng = np.random.RandomState(1)
    for n in (3, 4, 9):
        A = rng.normal(size=(5, n, n))
        A = A @ np.swapaxes(A, 1, 2)
        w, V = sr.jacobi_eigh(A)
        for k in range(5):
            assert np.abs(np.sort(w[k]) - np.linalg.eigvalsh(A[k])).max() <= 1e-12 * np.abs(w[k]).max()
            assert np.abs(V[k] @ np.diag(w[k]) @ V[k].T - A[k]).max() <= 1e-12 * np.abs(A[k]).max()


def test_restatement_sfm_drives_a_stream(vio, oracle_lib):
    """StreamDriver(initialize=dict(sfm=<callable>, aligner=...)) on the CPU oracle backend: the restatement's SfM feeds the alignment
    restatement, the window initialises at the first try and the run stays at the ground-truth start's accuracy.  Without `sfm` the
    driver is untouched: the SfM callable is never called."""
    import init_reference as ir
    from vio_amd import stream as vs
    mk = lambda: vs.SyntheticStream(n_frames=16, landmarks_per_frame=60, track_len=10, seed=3, pixel_noise=0.1 * PX)  # noqa: E731
    calls = []

    def sfm(items):
        calls.append(len(items))
        return [sr.sfm(it) for it in items]

    d0 = vs.StreamDriver(oracle_lib, mk(), seed=2)
    e0 = vs.ape_stats(d0.run(), d0.ground_truth())["rmse"]
    d = vs.StreamDriver(oracle_lib, mk(), seed=2, initialize=dict(sfm=sfm, aligner=ir.make_aligner(oracle_lib)))
    tr = d.run()
    assert calls == [1] and d.init_tries == 1 and d.init_sfm_status == [0] and d.init_result["status"] == 0
    e = vs.ape_stats(tr, d.ground_truth())["rmse"]
    assert e <= 0.01 and e0 <= 0.01, (e, e0)
    s_true = np.linalg.norm(sr.ground_truth(d.s, list(range(11)), 0, [])[3])
    assert abs(d.init_result["s"] / s_true - 1) <= 1e-2
    plain = vs.StreamDriver(oracle_lib, mk(), seed=2, initialize=dict(scale=3.7, aligner=ir.make_aligner(oracle_lib)))
    plain.ensure_initialized()
    assert calls == [1] and not plain.init_sfm_status
