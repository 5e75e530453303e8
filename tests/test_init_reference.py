"""The numpy restatement of the visual-inertial alignment (tests/init_reference.py) against the ground truth of this tree's streams, and
its quirks one by one.  CPU only: the LDLTs go through the oracle's vioo_ldlt_solve.

Measured here (CPU, the restatement):
  - SyntheticStream, frames 0..10, noise-free stand-in at scale 3.7: s_linear 3.699849, s 3.699848 (4e-5 relative: the mid-point
    rule's discretisation), |g_linear| 9.809998, gravity direction 6.3e-5, body velocities 2.5e-4 m/s, gyro bias 2.2e-7 rad/s;
  - MH_05 stretch (RealImuStream): s, |g|, g and velocities to 1e-11, gyro bias 2e-14;
  - a constant gyro bias of (0.02, -0.01, 0.015) rad/s injected into the synthetic stream's raw samples: recovered after one
    step to 2.1e-5 (solveGyroscopeBias is one Gauss-Newton step: the rest is the linearisation of delta_q in bg).
The bars are 10x or more above these numbers.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_reference as ir  # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = list(range(11))


def streams(vio):
    from vio_amd import stream as vs
    syn = vs.SyntheticStream(n_frames=14, seed=0)
    mh = vs.RealImuStream(dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz"))))
    return [("synthetic", syn, vio.synth.G_NORM, vio.synth.T_IC, vio.synth.R_IC), ("mh05", mh, mh.g_norm, mh.tic, mh.ric)]


def window(vio, st, scale=3.7, frames=FRAMES, **kw):
    from vio_amd import stream as vs
    R, T = vs.visual_trajectory(st, frames, 0, scale, **kw)
    return dict(R=R, T=T, pre=[st.preint[f] for f in frames[:-1]])


def truth(st, ric, tic, G, frames=FRAMES):
    Rcl = st.R[frames[0]] @ ric
    return Rcl.T @ np.array([0.0, 0.0, G]), np.concatenate([st.R[f].T @ st.V[f] for f in frames])


@pytest.mark.parametrize("which", ["synthetic", "mh05"])
def test_noise_free_window_recovers_scale_gravity_and_velocities(vio, oracle_lib, which):
    name, st, G, tic, ric = [s for s in streams(vio) if s[0] == which][0]
    item = window(vio, st)
    bg, status = ir.gyro_bias(oracle_lib, item, np.zeros(3))
    assert status == ir.OK
    out = ir.align(oracle_lib, item, tic, G, bg)
    assert out["status"] == ir.OK
    g_true, v_true = truth(st, ric, tic, G)
    tol = dict(synthetic=(5e-4, 1e-3, 1e-3, 5e-3, 1e-5), mh05=(1e-9, 1e-9, 1e-9, 1e-9, 1e-12))[which]
    assert abs(out["s_linear"] / 3.7 - 1) <= tol[0] and abs(out["s"] / 3.7 - 1) <= tol[0]
    assert abs(np.linalg.norm(out["g_linear"]) - G) <= tol[1]
    assert abs(np.linalg.norm(out["g"]) - G) <= 1e-12 * G        # RefineGravity keeps |g| = G by construction
    assert np.abs(out["g"] - g_true).max() <= tol[2] * G
    assert np.abs(out["x"][:33] - v_true).max() <= tol[3]
    assert np.abs(bg).max() <= tol[4]
    # the state change: g_world = (0, 0, G), positions relative to frame 0's body, yaw of frame 0 zeroed
    assert np.abs(out["g_world"] - [0, 0, G]).max() <= 1e-9 * G
    assert np.abs(out["poses"][0, 0:3]).max() == 0.0
    R0w = vio.synth.quat_to_rot(out["poses"][0, 3:7])
    assert abs(np.degrees(np.arctan2(R0w[1, 0], R0w[0, 0]))) <= 1e-9
    # speeds and distances are metric: the ground truth's, up to the rotation about gravity
    for k in range(11):
        assert abs(np.linalg.norm(out["speed_bias"][k, 0:3]) - np.linalg.norm(st.V[k])) <= tol[3] * 10
        assert abs(np.linalg.norm(out["poses"][k, 0:3]) - np.linalg.norm(st.P[k] - st.P[0])) <= tol[3] * 10
    assert np.all(out["speed_bias"][:, 3:6] == 0.0) and np.all(out["speed_bias"][:, 6:9] == bg)


def test_injected_gyro_bias_is_recovered_in_one_step(vio, oracle_lib):
    from vio_amd import stream as vs
    st = vs.SyntheticStream(n_frames=14, seed=0)
    b = np.array([0.02, -0.01, 0.015])
    pre = []
    for iv in st.imu[:10]:
        pre.append(vio.synth.preintegrate(iv["acc0"], np.asarray(iv["gyr0"]) + b, np.zeros(3), np.zeros(3), iv["dt"], iv["acc"],
                                          [np.asarray(g) + b for g in iv["gyr"]]))
    R, T = vs.visual_trajectory(st, FRAMES, 0, 3.7)
    bg, status = ir.gyro_bias(oracle_lib, dict(R=R, T=T, pre=pre), np.zeros(3))
    assert status == ir.OK
    assert np.abs(bg - b).max() <= 2e-4             # (measured 2.1e-5)


def test_failure_branches(vio, oracle_lib):
    name, st, G, tic, _ = streams(vio)[0]
    item = window(vio, st)
    bg, _ = ir.gyro_bias(oracle_lib, item, np.zeros(3))
    # T negated: the linear stage finds s < 0 with |g| right (the rotations still carry gravity)
    neg = dict(item, T=-np.asarray(item["T"]))
    out = ir.align(oracle_lib, neg, tic, G, bg)
    assert out["status"] == ir.FAIL_SCALE and out["s_linear"] < 0
    assert np.isnan(out["s"]) and np.all(np.isnan(out["poses"]))
    # gravity off by more than 1: the stated norm G is 3 away from what the IMU measures
    out = ir.align(oracle_lib, item, tic, G + 3.0, bg)
    assert out["status"] == ir.FAIL_GRAVITY and abs(np.linalg.norm(out["g_linear"]) - (G + 3.0)) > 1.0
    # a non-finite input
    bad = dict(item, T=np.array(item["T"], dtype=np.float64))
    bad["T"][3, 1] = np.nan
    assert ir.align(oracle_lib, bad, tic, G, bg)["status"] == ir.NOT_FINITE


def test_tangent_basis_is_orthonormal():
    rng = np.random.RandomState(3)
    cases = [[0.0, 0.0, 9.81], [0.0, 0.0, 1.0], [1e-9, 0.0, 9.81], [0.0, 1e-3, -9.81]] + [list(rng.normal(size=3) * 5) for _ in range(20)]
    for g in cases:
        B = np.array(ir.tangent_basis(g))
        a = np.asarray(g) / np.linalg.norm(g)
        M = np.column_stack([a, B])
        # (near +z, tmp - a (a . tmp) cancels: 1e-9 off the axis leaves 1.0e-10 of orthogonality, measured)
        assert np.abs(M.T @ M - np.eye(3)).max() <= (1e-9 if abs(g[2]) > 1e3 * abs(g[0]) + 1e3 * abs(g[1]) else 1e-14), g
    # the exact comparison: (0,0,1) takes tmp = (1,0,0), so b = (1,0,0), c = a x b = (0,1,0)
    assert ir.tangent_basis([0.0, 0.0, 9.81]) == [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]
    # ... and only (0,0,1): at (0,0,-1) tmp - a (a . tmp) vanishes and the basis degenerates to zero, as the reference's does
    assert ir.tangent_basis([0.0, 0.0, -9.81]) == [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]


def test_g2r_maps_gravity_to_z_with_zero_yaw():
    rng = np.random.RandomState(4)
    cases = [list(rng.normal(size=3)) for _ in range(20)] + [[0.0, 0.0, -9.81], [1e-14, 0.0, -9.81], [0.0, 3e-13, -1.0],
                                                             [0.0, 0.0, 9.81]]
    for g in cases:
        R = np.array(ir.g2r(g))
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
        z = R @ (np.asarray(g) / np.linalg.norm(g))
        assert np.abs(z - [0, 0, 1]).max() <= 1e-12, (g, z)
        assert abs(np.arctan2(R[1, 0], R[0, 0])) <= 1e-12
    # the antiparallel branch (FromTwoVectors' c < -1 + 1e-12): taken for -z and for vectors within 1e-12 of it
    for g in ([0.0, 0.0, -9.81], [1e-14, 0.0, -9.81], [0.0, 3e-13, -1.0]):
        assert ir.from_two_vectors_z(ir.normalized(g))[1]
    assert not ir.from_two_vectors_z([0.0, 1e-5, -1.0])[1]
    # exactly -z: the QR's null vector is (1, 0, 0), a half turn about x
    R, _ = ir.from_two_vectors_z([0.0, 0.0, -1.0])
    assert np.allclose(R, np.diag([1.0, -1.0, -1.0]), atol=1e-15)


def test_velocity_index_quirk_with_non_keyframes(vio, oracle_lib):
    """Keyframe kv's velocity is read from x.segment<3>(kv * 3) (estimator.cpp:428-435), an all-frame index: with non-keyframes
    between, keyframe 1 gets frame 1's body velocity rotated by keyframe 1's rotation, not its own."""
    name, st, G, tic, ric = streams(vio)[1]
    frames = list(range(8))
    item = window(vio, st, frames=frames)
    item["is_key"] = np.array([1, 0, 1, 1, 0, 1, 1, 1], dtype=bool)
    out = ir.align(oracle_lib, item, tic, G, np.zeros(3))
    assert out["status"] == ir.OK and out["n_key"] == 6
    keys = [0, 2, 3, 5, 6, 7]
    x = out["x"]
    for kv, f in enumerate(keys):
        V = out["rot"] @ (np.asarray(item["R"][f]) @ x[3 * kv:3 * kv + 3])
        assert np.abs(out["speed_bias"][kv, 0:3] - V).max() <= 1e-12
    assert np.abs(out["speed_bias"][1, 0:3] - out["rot"] @ (np.asarray(item["R"][2]) @ x[6:9])).max() > 1e-3


def test_refine_system_accumulates_across_iterations(vio, oracle_lib, monkeypatch):
    """RefineGravity zeroes A and b once, before its loop (initial_aligment.cpp:63-66): iteration k solves
    1000^(k+1) C_0 + ... + 1000 C_k.  The restatement keeps that: the system of the last solve is dominated by the first iteration's."""
    name, st, G, tic, _ = streams(vio)[0]
    item = window(vio, st)
    seen = []
    real = ir._solve_lower
    monkeypatch.setattr(ir, "_solve_lower", lambda lib, A, b: seen.append(np.array(A)[-1][-1]) or real(lib, A, b))
    ir.align(oracle_lib, item, tic, G, np.zeros(3))
    assert len(seen) == 5
    assert all(seen[k + 1] / seen[k] > 999.0 for k in range(1, 4))


def test_constructed_windows_take_the_exact_branches(vio, oracle_lib):
    """Gravity exactly on +z in the SfM frame: TangentBasis's exact a == (0,0,1) branch; exactly on -z: its degenerate basis and
    FromTwoVectors' antiparallel branch; gravity 0.9 above the stated G: the linear stage passes and the refined scale is negative."""
    tic = (0.05, 0.04, 0.03)
    up, tr = ir.vertical_window(down=False)
    out = ir.align(oracle_lib, up, tic, 9.81, np.zeros(3))
    assert out["status"] == ir.OK and list(out["g_linear"][:2]) == [0.0, 0.0] and ir.normalized(list(out["g_linear"])) == [0.0, 0.0, 1.0]
    assert abs(out["s"] / tr["scale"] - 1) <= 1e-9 and np.abs(out["x"][:33] - tr["v"].ravel()).max() <= 1e-9
    down, tr = ir.vertical_window(down=True)
    out = ir.align(oracle_lib, down, tic, 9.81, np.zeros(3))
    assert out["status"] == ir.OK and ir.normalized(list(out["g"])) == [0.0, 0.0, -1.0]
    assert ir.from_two_vectors_z(ir.normalized(list(out["g"])))[1]
    assert np.abs(out["g_world"] - [0, 0, 9.81]).max() <= 1e-12 and abs(out["s"] / tr["scale"] - 1) <= 1e-9
    heavy, _ = ir.vertical_window(g_true=9.81 + 0.9)
    out = ir.align(oracle_lib, heavy, tic, 9.81, np.zeros(3))
    assert out["status"] == ir.FAIL_REFINED_SCALE and out["s_linear"] > 0 and out["s"] < 0      # (measured 2.0 and -1.49)
    assert np.all(np.isfinite(out["x"])) and np.all(np.isnan(out["poses"]))


def test_near_antiparallel_branch_on_mh05(vio, oracle_lib):
    """MH_05's window seen from an SfM frame whose z axis points along gravity's opposite: the estimate is within 1e-11 of -z, so
    FromTwoVectors takes its antiparallel branch with a non-trivial null vector, and the state change still ends at g_world = (0,0,G)."""
    name, st, G, tic, ric = streams(vio)[1]
    item = window(vio, st)
    g_true, _ = truth(st, ric, tic, G)
    rot = ir.rotate_window(item, ir.rotation_onto(g_true / np.linalg.norm(g_true), [0.0, 0.0, -1.0]))
    out = ir.align(oracle_lib, rot, tic, G, np.zeros(3))
    a = ir.normalized(list(out["g"]))
    assert out["status"] == ir.OK and a != [0.0, 0.0, -1.0] and ir.from_two_vectors_z(a)[1]
    assert np.abs(out["g_world"] - [0, 0, G]).max() <= 1e-9 * G
    ref = ir.align(oracle_lib, item, tic, G, np.zeros(3))
    assert abs(out["s"] - ref["s"]) <= 1e-9 and np.abs(out["speed_bias"] - ref["speed_bias"]).max() <= 1e-8


def test_restatement_aligner_drives_a_stream(vio, oracle_lib):
    """StreamDriver(initialize=dict(aligner=...)) with the restatement on the CPU oracle backend: initialises on the first try and
    tracks as closely as the ground-truth start (aligned APE measured 0.0033 m against 0.0018 m)."""
    from vio_amd import stream as vs
    d0 = vs.StreamDriver(oracle_lib, vs.SyntheticStream(n_frames=20, seed=3), seed=2)
    e0 = vs.ape_stats(d0.run(), d0.ground_truth())["rmse"]
    d = vs.StreamDriver(oracle_lib, vs.SyntheticStream(n_frames=20, seed=3), seed=2,
                        initialize=dict(scale=3.7, aligner=ir.make_aligner(oracle_lib)))
    tr = d.run()
    assert d.init_tries == 1 and d.init_frame == 10 and abs(d.init_result["s"] / 3.7 - 1) <= 1e-3
    assert len(tr) == len(d0.trajectory)
    assert vs.ape_stats(tr, d.ground_truth())["rmse"] <= max(3 * e0, 0.01)


def test_initialize_batched_groups_mixed_drivers(vio, oracle_lib):
    """A synthetic and an MH_05 driver (different extrinsic, G and IMU noise) initialised together: one aligner call per group per
    round, each with its own drivers' tic / G / noise, and the same result as each driver alone."""
    from vio_amd import batch_stream, stream as vs
    base = ir.make_aligner(oracle_lib)
    calls = []

    def aligner(items, intervals, tic, g_norm, noise):
        calls.append((len(items), tuple(tic), g_norm))
        return base(items, intervals, tic, g_norm, noise)
    mh = dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))
    mk = [lambda: vs.SyntheticStream(n_frames=14, seed=3), lambda: vs.RealImuStream(mh, landmarks_per_frame=30, seed=7)] * 2
    cfgs = [dict(scale=3.7, aligner=aligner), dict(scale=3.7, aligner=aligner), dict(scale=2.0, rot_noise=1e-3, seed=1, aligner=aligner),
            dict(scale=2.0, rot_noise=1e-3, seed=1, aligner=aligner)]
    drivers = [vs.StreamDriver(oracle_lib, m(), seed=2, initialize=c) for m, c in zip(mk, cfgs)]
    assert batch_stream.initialize_batched(drivers) == 1
    assert sorted(calls) == sorted([(2, tuple(vio.synth.T_IC), vio.synth.G_NORM), (2, tuple(drivers[1].s.tic), drivers[1].s.g_norm)])
    for m, c, d in zip(mk, cfgs, drivers):
        alone = vs.StreamDriver(oracle_lib, m(), seed=2, initialize=dict(c, aligner=base))
        alone.ensure_initialized()
        assert alone.init_result["s"] == d.init_result["s"] and np.array_equal(alone.poses, d.poses)
