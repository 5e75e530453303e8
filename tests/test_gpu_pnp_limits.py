"""The batched PnP (include/vio_pnp.h, k_pnp_frames) where its Levenberg-Marquardt loop leaves the easy path, against the numpy
restatement (tests/pnp_reference.py, order "wave64").  tests/test_gpu_pnp.py sends frames that run 3 or 4 iterations, accept every
step and leave by the step or the gradient tolerance; this file sends the rest: rejected steps and the doubling of vv, the reset of vv
on the next accept, the 20-iteration cap, failed factorisations, the radius floor, the gradient test at the guess, the clamp of the
damping diagonal, rotation steps of radians, the three `trace <= 0` branches of rot_to_quat, and wavefronts of one workgroup that end
after 0, 4, 17 and 20 iterations.

The rule is test_gpu_pnp._compare's, unchanged: statuses, n_used and iteration counts identical; Q, T and cost inside 10x the
restatement's own spread under two one-ulp perturbations of the image points plus 1e-13 of the quantity's size; a frame whose
restatement iteration count moves under that perturbation is undecidable.  The cap here is zero undecidable frames.  The cases live
in pnp_reference.LIMIT_CASES; every test first asserts on the restatement's trace that the branch the case is named after is taken
(pnp_reference.check_limit_case), and tests/test_pnp_reference.py holds the same, and the zero, on the CPU.

Chosen on the CPU (one letter per iteration: A accept, R reject, C failed factorisation, S step tolerance):
    far_frame(40, seed, rot, tr=1)    rot 0.8: seed 1 RRRRAAAAAAAAS (13), seed 2 R{5}A{12}S (18), seed 3 R{6}A{14} (the cap, at 20);
                                      rot 1.5: seed 2 RRRRRARAAARARRAARRRA, seed 5 RRRRRARAAAAAAAAAAAAR; rot 2.5: seed 1
                                      RRRRARRRAAAAAARARRRA, seed 3 AAAARRRRRAAAAAAAAAAA; rot 3.1: seed 1 RRRRRRAAAAAAARRRAAAA, seed 5
                                      ARRRRARRAAAAAAAAAAAA; all at the cap, 5 to 12 rejects, final costs 0.8 to 1.1e5
    shallow (depth 0.05 to 0.3)       seed 1 RRRRRRAAARAAAAAAAARR, seed 2 ARRRRRARAAAAAAAAAARA: 9 and 7 rejects, the cap
    points x 1e6, 1e12, 1e150         13, 5 and 4 iterations, diagmin in every one
    one point at (z, z, z)            z 1e-120: C{7}AC{6}S (15), AC{16} (the radius floor at 17), CCAC{15} (the floor at 18);
                                      z 1e-150: C{6}AC{8}S (16), C{5}AC{14} (the floor, at 20); z 1e-154: C{15}, the floor with no
                                      accepted step: the pose is the guess, the cost the first
    image points x 1e100, x 1e160     R{15} to the floor at cost 9.0e199; FAIL_NO_POSE at 0 iterations
    near_frame(24, 5, axis, angle)    3 iterations, trace of the result -0.17 to -1.0, rot_to_quat's else branch with i = axis
    noise-free far_frame, rot 0.3/0.8 the restatement's own distance to the pose the frame was made from, R / T (max-norm): rot 0.3
                                      seed 1 6.2e-9 / 4.0e-8, seed 7 1.9e-9 / 1.5e-8; rot 0.8 seed 1 3.2e-9 / 2.0e-8, seed 7 3.1e-9 /
                                      2.9e-8; the device is held to 10x that plus 1e-13
The seeds of the frames with a point at (z, z, z) were picked so that the count also stays put under 20 further one-ulp draws and
under one ulp of the step's rotation: where a pivot's sign hangs on the last bit of a 1e240 cancellation most seeds do not.

Measured on an MI355X, every frame decidable and every status and iteration count the restatement's: the device's Q, T and cost are
the restatement's bit for bit (error 0, ratio 0) in every case of the groups shallow, zero, diagmin, cholfail, quat, guess, truth and
sizes and in every window of several frames.  The largest error over its bar elsewhere: reject 0.032 (far_rot2.5_seed1, cost: 1.6e-11
against 5.0e-10; Q at most 6.9e-16 against bars of 1.0e-13 to 3.7e-12), the four fates 0.0018 (the same capped frame inside the
windows).  The four frames that differ at all are runs at the cap whose steps are rotations of radians, where sin and cos come from
another library than the restatement's.  Against the pose the frame was made from the device's distance is the restatement's to all
four printed digits (R 1.9e-9 to 6.2e-9, T 1.5e-8 to 4.0e-8, bars ten times those).  The zero-iteration frames return the guess to
1.4e-17 (Q) and 5.6e-17 (T).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_reference as pr  # noqa: E402
import sfm_reference as sr  # noqa: E402
from test_gpu_pnp import _bits, _compare, _frame_bits, pnp_lib  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SOLO = [n for n, c in pr.LIMIT_CASES.items() if c["cfg"] is None]       # the one-frame cases at the default min_points
ROUND_TRIP = 16 * 2.0 ** -53        # quaternion -> matrix -> quaternion: a dozen roundings of quantities of size one


@pytest.fixture(scope="module")
def handle(pnp_lib):
    return pnp_lib.create()


@pytest.fixture(scope="module")
def solo(handle):
    """Every one-frame case as a window of its own, all in one call: name -> the device's window."""
    return dict(zip(SOLO, handle.frames_batch([pr.limit_case(n)[0] for n in SOLO])))


def _held(got, name):
    item, cfg, ref, trace = pr.check_limit_case(name)
    assert _compare(got, item, "%s:%s" % (pr.LIMIT_CASES[name]["group"], name)) == 0
    return item, ref, trace


@pytest.mark.parametrize("name", [n for n in SOLO if pr.LIMIT_CASES[n]["group"] in ("reject", "shallow", "diagmin", "guess")])
def test_rejected_steps_cap_and_clamp(solo, name):
    _, ref, _ = _held(solo[name], name)
    assert solo[name]["status"] == pr.OK and solo[name]["iterations"][0] == ref["iterations"][0]


@pytest.mark.parametrize("name", [n for n in SOLO if pr.LIMIT_CASES[n]["group"] == "zero"])
def test_zero_iterations_with_a_pose(solo, name):
    item, _, trace = _held(solo[name], name)
    got = solo[name]
    assert trace == ["grad0"] and got["status"] == pr.OK and got["iterations"][0] == 0 and np.isfinite(got["cost"][0])
    eq, et = np.abs(got["Q"][0] - item["key_Q"][0]).max(), np.abs(got["T"][0] - item["key_T"][0]).max()
    print("%s: the guess comes back to %.2e / %.2e, bar %.2e" % (name, eq, et, ROUND_TRIP))
    assert eq <= ROUND_TRIP and et <= ROUND_TRIP * max(1.0, np.abs(item["key_T"]).max())


@pytest.mark.parametrize("name", [n for n in SOLO if pr.LIMIT_CASES[n]["group"] == "cholfail"])
def test_failed_factorisations_and_radius_floor(solo, name):
    item, ref, trace = _held(solo[name], name)
    got = solo[name]
    if name == "obs_x1e160":
        assert (got["status"], got["fail_frame"], got["iterations"][0]) == (pr.FAIL_NO_POSE, 0, 0) and trace == ["nocost"]
    elif "accept" not in trace:         # the floor with no accepted step: the guess (the identity) and the cost at it
        assert trace[-1] == "radmin" and got["status"] == pr.OK
        assert np.array_equal(got["Q"][0], [1.0, 0.0, 0.0, 0.0]) and np.all(got["T"][0] == 0.0)


@pytest.mark.parametrize("name", [n for n in SOLO if pr.LIMIT_CASES[n]["group"] == "quat"])
def test_output_rotations_above_120_degrees(solo, name):
    _, ref, _ = _held(solo[name], name)
    axis = pr.LIMIT_CASES[name]["quat"]
    R = sr.quat_to_rot(ref["Q"][0])
    assert np.trace(R) <= 0 and pr.quat_branch(R) == axis and int(np.argmax(np.abs(solo[name]["Q"][0]))) == 1 + axis
    print("%s: trace %.3f, w %.3e" % (name, np.trace(R), solo[name]["Q"][0][0]))


@pytest.mark.parametrize("name", [n for n in SOLO if pr.LIMIT_CASES[n]["group"] == "truth"])
def test_against_the_pose_the_frame_was_made_from(solo, name):
    """The one check that does not share the restatement's formulae for the optimum; the bar is 10x the restatement's own distance
    to that pose on the same frame plus 1e-13 (the committed values: the module docstring)."""
    item, ref, _ = _held(solo[name], name)
    got = solo[name]
    Rt = sr.quat_to_rot(item["true_Q"])
    for key, g, r, t in (("R", sr.quat_to_rot(got["Q"][0]), sr.quat_to_rot(ref["Q"][0]), Rt), ("T", got["T"][0], ref["T"][0], item["true_T"])):
        own, err = float(np.abs(r - t).max()), float(np.abs(g - t).max())
        print("truth:%-20s %s err %.3e  restatement's %.3e  bar %.3e" % (name, key, err, own, 10.0 * own + 1e-13))
        assert err <= 10.0 * own + 1e-13, (name, key, err, own)


def test_one_workgroup_four_fates(handle, solo):
    w = pr.limit_windows()
    for n in pr.FOUR_FATES:
        pr.check_limit_case(n)
    alone = [solo[n] for n in pr.FOUR_FATES]
    its = [int(a["iterations"][0]) for a in alone]
    assert its[0] == 0 and 3 <= its[1] <= 4 and its[2] == 20 and its[3] not in its[:3]
    one, again = handle.frames_batch([w["four_fates"]])[0], handle.frames_batch([w["four_fates"]])[0]
    perm = handle.frames_batch([w["four_fates_permuted"]])[0]
    seven = handle.frames_batch([w["four_fates_straddling"]])[0]
    assert _bits(one) == _bits(again)
    for k in range(4):
        bits = _frame_bits(alone[k], 0)
        assert bits == _frame_bits(one, k) == _frame_bits(perm, pr.FATES_PERMUTED.index(k)) == _frame_bits(seven, 3 + k), k
    for name in ("four_fates", "four_fates_permuted", "four_fates_straddling"):
        got = dict(four_fates=one, four_fates_permuted=perm, four_fates_straddling=seven)[name]
        assert got["status"] == pr.OK and _compare(got, w[name], "fates:" + name) == 0
    # a frame without observations between two solvable ones: the scratch offsets behind it hold
    got = handle.frames_batch([w["empty_between"]])[0]
    assert (got["status"], got["fail_frame"], got["n_used"][1]) == (pr.FAIL_FEW_POINTS, 1, 0)
    assert _frame_bits(got, 0) == _frame_bits(alone[1], 0) and _frame_bits(got, 2) == _frame_bits(alone[2], 0)
    assert _compare(got, w["empty_between"], "fates:empty_between") == 0


def test_accepted_sizes_at_the_edge(handle, solo, monkeypatch):
    # exactly VIO_PNP_MAX_FRAMES frames
    syn = pr.fixture("syn")["item"]
    ten, full = handle.frames_batch([syn, pr.limit_windows()["full_window"]])
    assert len(full["Q"]) == pr.MAX_FRAMES == 32 and full["status"] == pr.OK
    for k in range(pr.MAX_FRAMES):
        assert _frame_bits(full, k) == _frame_bits(ten, k % 10), k
    assert _compare(full, pr.limit_windows()["full_window"], "sizes:full_window") == 0
    # a point seen twice
    _held(solo["point_twice"], "point_twice")
    # min_points at both ends of its range
    try:
        for name, short in (("three_points", pr.synthetic_frame(2, 5)), ("max_points", pr.synthetic_frame(pr.MAX_POINTS - 1, 3))):
            item, cfg, ref, _ = pr.check_limit_case(name)
            handle.set_config(**cfg)
            got, few = handle.frames_batch([item, short])
            monkeypatch.setitem(pr.DEFAULT_CFG, "min_points", cfg["min_points"])        # (_compare's restatement runs at the default)
            assert got["status"] == pr.OK and got["n_used"][0] == cfg["min_points"] and _compare(got, item, "sizes:" + name) == 0
            assert (few["status"], few["fail_frame"], few["n_used"][0]) == (pr.FAIL_FEW_POINTS, 0, cfg["min_points"] - 1)
    finally:
        handle.set_config()
