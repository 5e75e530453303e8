"""The residual query's reference (tests/res_reference.py, built on the oracle's exported pieces) against the oracle itself: its chi2
breakdown adds up to the oracle context's vio_chi2 under every loss, with the extrinsic fixed and free, for XYZ landmarks, with a
marginalisation prior and with an IMU edge missing; and on the seeded outlier window its flags meet the recall and precision the GPU
tests hold the library to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import res_reference as rr  # noqa: E402


@pytest.mark.parametrize("case", rr.CASES, ids=[c[0] for c in rr.CASES])
def test_breakdown_adds_up_to_the_oracle_chi2(vio, oracle_lib, case):
    w, kw = rr.make_case(vio, oracle_lib, case)
    c = oracle_lib.context(**kw)
    c.load(w)
    c.solve(5)
    obs, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w)
    chi = c.chi2()
    assert abs(s["chi2"] - chi) <= 1e-12 * abs(chi), (s["chi2"], chi)
    assert s["imu"] == s["imu_edge"].sum()
    if case[6] is not None:
        assert s["imu_edge"][case[6]] == 0.0
    assert (s["prior"] > 0) == bool(case[4])
    assert s["frame_edges"].sum() == len(w.lm)
    assert np.isclose(s["frame_robust"].sum(), s["visual_robust"], rtol=1e-12)
    if kw["loss_type"] == 0:
        assert np.array_equal(obs[:, 2], obs[:, 3])              # no loss: rho0 is e2
    else:
        assert np.all(obs[:, 3] <= obs[:, 2] * (1 + 1e-15))      # the robust losses only shrink
    assert not flags.any()                                        # a clean window: nothing to flag


def test_no_imu_gives_nan(vio, oracle_lib):
    w, kw = rr.make_case(vio, oracle_lib, rr.CASES[2])
    c = oracle_lib.context(**kw)
    c.load(w)
    _, _, _, s = rr.reference_of(oracle_lib, vio, c, w, imu=False)
    assert np.isnan(s["chi2"]) and np.isnan(s["imu"]) and np.all(np.isnan(s["imu_edge"]))
    assert np.isfinite(s["visual_robust"])


def test_seeded_outliers_recall_and_precision(vio, oracle_lib):
    w, truth = rr.outlier_window(vio)
    assert truth.sum() == 100
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(10)
    _, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w, outlier_px=3.0)
    recall, precision = rr.recall_precision(flags, truth)
    assert recall >= rr.RECALL_MIN and precision >= rr.PRECISION_MIN, (recall, precision)
    assert s["n_flagged"][0] == np.count_nonzero(flags & 1)
    # the margins the thresholds rest on
    assert lmo[~truth, 0].max() < 2.5 and lmo[truth, 0].min() > 9.0


def test_flag_rules_on_a_broken_state(vio, oracle_lib):
    """Bit 1 (a point behind the observing camera) and bit 2 (an inverse depth that is not positive and finite)."""
    w = vio.synth.make_window(30, seed=5)
    c = oracle_lib.context()
    c.load(w)
    poses, sb, ext = c.get_window()
    vals = np.array(c.get_landmarks())
    vals[3], vals[7] = -vals[3], np.nan
    _, err = c.get_prior()
    # (the initial state is unsolved: bit 0 is kept out of the way with a threshold no clean landmark reaches)
    _, lmo, flags, s = rr.reference(oracle_lib, vio, c.cfg, w, poses, sb, ext, vals, err, outlier_px=1e4)
    assert flags[3] & 2 and flags[3] & 4                         # negative depth: behind every camera, and solve_flag = 2
    assert flags[7] == 5                                          # NaN: the mean error is NaN too (a NaN depth is not <= 0)
    assert np.isnan(lmo[7, 0]) and np.isnan(lmo[7, 1])
    assert not np.delete(flags, [3, 7]).any()
    assert list(s["n_flagged"]) == [int(flags[3] & 1) + 1, 1, 2]
