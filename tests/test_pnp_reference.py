"""The numpy restatement of the non-keyframe PnP (tests/pnp_reference.py) and the Python helpers around the library, on the CPU.

The fixtures are the 10 non-keyframes of the 21-frame synthetic window and of the MH_05 window (pnp_reference.fixture: first = 0, no
other `first` had to be tried); the points come from sfm_reference.sfm on the 11 keyframes.  Each pose is held to the stream's ground
truth in frame l at the SfM's scale.  The bar is 10 x the largest error (over the 10 frames, Q up to sign and T, max-norm) the
restatement itself shows on that window, measured here on the CPU:
    synthetic, noise-free   7.9e-9    bar 7.9e-8          synthetic, 0.1 px   6.2e-4    bar 6.2e-3
    MH_05, noise-free       6.5e-8    bar 6.5e-7          MH_05, 0.1 px       3.6e-3    bar 3.6e-2
(the noise-free error is what the keyframes' bundle adjustment leaves when it stops at Ceres' tolerances).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_reference as pr  # noqa: E402
import sfm_reference as sr  # noqa: E402

BARS = {("syn", False): 7.9e-8, ("mh", False): 6.5e-7, ("syn", True): 6.2e-3, ("mh", True): 3.6e-2}


def _frame_problem(item, k):
    off = item["obs_offset"]
    op, ob = item["obs_point"][off[k]:off[k + 1]], item["obs_pts"][off[k]:off[k + 1]]
    use = item["valid"][op]
    g = item["guess_key"][k]
    R0, t0 = pr.guess_pose(item["key_Q"][g], item["key_T"][g])
    return R0, t0, item["points"][op[use]], ob[use]


@pytest.mark.parametrize("which", ["syn", "mh"])
def test_sequential_order_is_the_sfm_restatement_bit_for_bit(which):
    item = pr.fixture(which)["item"]
    n = 0
    for k in range(len(item["guess_key"])):
        R0, t0, X, obs = _frame_problem(item, k)
        if len(X) < sr.PNP_MIN_POINTS:
            continue
        a = sr.solve_frame_by_pnp(R0, t0, X, obs)
        b = pr.solve(R0, t0, X, obs, order="sequential")
        assert a[0] == b[0] and a[3] == b[3] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), k
        n += 1
    assert n == 10


def test_wave_sum_is_lane_strided_then_butterfly():
    rng = np.random.RandomState(1)
    for n in (1, 6, 63, 64, 65, 128, 129, 300):
        x = rng.normal(size=(n, 3)) * 10.0 ** rng.randint(-8, 8, (n, 3))
        lanes = [[0.0] * 3 for _ in range(64)]
        for m in range(n):
            for c in range(3):
                lanes[m % 64][c] = lanes[m % 64][c] + x[m, c]
        s = 1
        while s < 64:
            lanes = [[lanes[i][c] + lanes[i ^ s][c] for c in range(3)] for i in range(64)]
            s *= 2
        assert all(lanes[i] == lanes[0] for i in range(64))
        assert list(pr._wave_sum(x)) == lanes[0], n


@pytest.mark.parametrize("which,noisy", [("syn", False), ("mh", False), ("syn", True), ("mh", True)])
def test_wave64_order_against_ground_truth(which, noisy):
    fx = pr.fixture(which, noisy)
    out = pr.frames(fx["item"])
    assert out["status"] == pr.OK and len(out["Q"]) == 10 and np.all(out["frame_status"] == pr.OK)
    Qg, Tg = pr.ground_truth_frames(fx["stream"], fx["win"], fx["sfm"]["rel"]["l"])
    eq = np.minimum(np.abs(out["Q"] - Qg).max(axis=1), np.abs(out["Q"] + Qg).max(axis=1))
    et = np.abs(out["T"] - Tg).max(axis=1)
    print(which, noisy, "errQ %.3e errT %.3e bar %.1e" % (eq.max(), et.max(), BARS[(which, noisy)]), "iterations", out["iterations"])
    assert max(eq.max(), et.max()) <= BARS[(which, noisy)]          # every frame: none is left out
    assert np.all(out["n_used"] >= 60) and np.all(out["iterations"] >= 1)


def test_one_ulp_leaves_the_iteration_counts_decidable():
    """The device comparison (tests/test_gpu_pnp.py) may skip a frame whose iteration count changes under one ulp, at most 2 of the 20:
    the restatement alone stays within that cap for the committed seeds."""
    changed = 0
    for which in ("syn", "mh"):
        item = pr.fixture(which)["item"]
        ref = pr.frames(item)
        rng = np.random.RandomState(5)
        runs = [pr.frames(pr.perturb_ulp(item, rng)) for _ in range(2)]
        changed += int(np.sum(np.any([r["iterations"] != ref["iterations"] for r in runs], axis=0)))
    print("frames whose count changes under one ulp:", changed)
    assert changed <= 2


def _reference_loop(stamps, headers):
    """estimator.cpp:312-327, literally: i walks Headers while frame_it walks all_image_frame."""
    out, i = [], 0
    for stamp in stamps:
        if stamp == headers[i]:
            i += 1
            continue
        if stamp > headers[i]:
            i += 1
        out.append(i)
    return out


def test_guess_key_is_the_references_rule(vio):
    from vio_amd import pnp
    stamps = [0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.45, 0.5, 0.55, 0.6]
    headers = [0.0, 0.1, 0.3, 0.4, 0.6]
    key = [s in headers for s in stamps]
    assert list(pnp.guess_keys(key)) == _reference_loop(stamps, headers) == [1, 2, 2, 2, 4, 4, 4]
    for bad in ([False, True, True], [True, False], []):
        with pytest.raises(ValueError):
            pnp.guess_keys(bad)
    fx = pr.fixture("syn")
    assert list(fx["item"]["guess_key"]) == list(range(1, 11))
    with pytest.raises(ValueError):
        vio.pnp_items_from_sfm([fx["sfm"]], [fx["win"]["sfm_item"]], [fx["win"]["all_frames"][1:]])


def test_init_items_of_all_frames(vio):
    fx = pr.fixture("syn")
    win, res = fx["win"], fx["sfm"]
    ric = vio.synth.quat_to_rot(fx["stream"].ext[3:7])
    # no non-keyframes: sfm_items_to_init_items' result, exactly
    kpres = [dict(sum_dt=float(k)) for k in range(10)]
    a = vio.all_frames_to_init_items([res], [None], ric, [kpres], [[1] * 11])[0]
    b = vio.sfm_items_to_init_items([res], ric, [kpres], is_key=[1] * 11)[0]
    assert sorted(a) == sorted(b) and a["pre"] == b["pre"] and a["is_key"] == b["is_key"]
    assert a["R"].tobytes() == b["R"].tobytes() and a["T"].tobytes() == b["T"].tobytes()
    empty = dict(status=0, Q=np.zeros((0, 4)), T=np.zeros((0, 3)))
    c = vio.all_frames_to_init_items([res], [empty], ric, [kpres], [[1] * 11])[0]
    assert c["R"].tobytes() == b["R"].tobytes()
    # with them: time order, is_key, the keyframes' rows the SfM's, the others' the PnP's
    out = pr.frames(fx["item"])
    it = vio.all_frames_to_init_items([res], [out], ric, [win["pres"]], [win["is_key"]])[0]
    assert it["is_key"] == [1, 0] * 10 + [1] and it["R"].shape == (21, 3, 3) and len(it["pre"]) == 20
    assert np.array_equal(it["T"][0::2], res["T"]) and np.array_equal(it["T"][1::2], out["T"])
    assert np.array_equal(it["R"][0::2], b["R"])
    assert np.array_equal(it["R"][3], vio.sfm.quat_wxyz_to_rot(out["Q"][1]) @ ric.T)
    # the non-keyframes lie between their neighbours
    for k in range(1, 20, 2):
        assert np.linalg.norm(it["T"][k] - 0.5 * (it["T"][k - 1] + it["T"][k + 1])) < 0.2 * np.linalg.norm(it["T"][k + 1] - it["T"][k - 1]) + 1e-3
    bad = dict(out, status=pr.FAIL_FEW_POINTS)
    assert vio.all_frames_to_init_items([res], [bad], ric, [win["pres"]], [win["is_key"]]) == [None]


def test_statuses():
    item = pr.fixture("syn")["item"]
    off = item["obs_offset"]
    usable = [np.nonzero(item["valid"][item["obs_point"][off[k]:off[k + 1]]])[0] for k in range(10)]

    def cut(k, n):            # frames 0 .. 9 with frame k cut to its first n usable observations
        op, ob, o = [], [], [0]
        for f in range(10):
            keep = usable[f][:n] if f == k else np.arange(off[f + 1] - off[f])
            op.append(item["obs_point"][off[f]:off[f + 1]][keep]); ob.append(item["obs_pts"][off[f]:off[f + 1]][keep]); o.append(o[-1] + len(keep))
        return dict(item, obs_offset=np.array(o, dtype=np.int64), obs_point=np.concatenate(op), obs_pts=np.concatenate(ob))

    whole = pr.frames(item)
    five = pr.frames(cut(4, 5))
    assert (five["status"], five["fail_frame"]) == (pr.FAIL_FEW_POINTS, 4) and five["n_used"][4] == 5 and np.all(np.isnan(five["Q"][4]))
    for k in (3, 5, 9):         # the frames after a failing one are still computed
        assert five["frame_status"][k] == pr.OK and five["Q"][k].tobytes() == whole["Q"][k].tobytes()
    six = pr.frames(cut(4, 6))
    assert six["status"] == pr.OK and six["n_used"][4] == 6 and np.all(np.isfinite(six["Q"][4]))
    assert pr.frames(cut(4, 6), dict(min_points=7))["fail_frame"] == 4
    # a frame whose points are all invalid
    valid = item["valid"].copy()
    valid[item["obs_point"][off[0]:off[1]]] = False
    inv = pr.frames(dict(item, valid=valid))
    assert (inv["status"], inv["fail_frame"], inv["n_used"][0]) == (pr.FAIL_FEW_POINTS, 0, 0)
    # a NaN observation: the whole window, and nothing but NaN
    ob = item["obs_pts"].copy()
    ob[off[2] + 1, 0] = np.nan
    nan = pr.frames(dict(item, obs_pts=ob))
    assert nan["status"] == pr.NOT_FINITE and nan["fail_frame"] == -1 and np.all(np.isnan(nan["Q"])) and np.all(nan["frame_status"] == pr.NOT_FINITE)
    # ... but the NaN coordinates of a point that is not valid are never read (vio_sfm_batch leaves them)
    assert np.any(~item["valid"]) and np.all(np.isnan(item["points"][~item["valid"]])) and whole["status"] == pr.OK
    # a point in the guess camera's z = 0 plane: the solve cannot start
    flat = pr.synthetic_frame(8, 1)
    flat["points"][3, 2] = 0.0
    r = pr.frames(flat)
    assert (r["status"], r["fail_frame"], r["iterations"][0]) == (pr.FAIL_NO_POSE, 0, 0) and np.all(np.isnan(r["T"]))
    assert pr.frames(pr.synthetic_frame(8, 1))["status"] == pr.OK


def test_limit_cases_take_their_branches():
    """What tests/test_gpu_pnp_limits.py sends to the device, on the restatement alone: every case takes the branches it is there
    for (pnp_reference.LIMIT_CASES), no frame of any case or window changes its iteration count under one ulp, so the device
    comparison skips none, and together the cases reach every way out of the loop.  A changed seed or constant fails here first."""
    seen, shapes, skipped = set(), {}, 0
    for name, c in pr.LIMIT_CASES.items():
        item, cfg, ref, trace = pr.check_limit_case(name)
        seen |= set(trace)
        shapes[name] = pr.shape(trace)
        if c["quat"] is not None:
            seen.add("quat%d" % c["quat"])
        skipped += pr.undecidable(item, cfg)
    windows = pr.limit_windows()
    skipped += sum(pr.undecidable(w) for w in windows.values())
    print("undecidable frames:", skipped)
    assert skipped == 0
    assert seen >= set(pr.EVENTS) - {"c2_not_finite", "model_not_positive"} | {"quat0", "quat1", "quat2"}, seen
    # consecutive rejects, then a reject behind a later accept (vv was reset); a converged run with at least four rejects; the
    # radius floor with and without an accepted step, by failed factorisations and by rejected steps
    assert any("RRA" in s and "AR" in s for s in shapes.values())
    assert any(s.count("R") >= 4 and pr.limit_case(n)[3][-1] == "steptol" for n, s in shapes.items())
    floor = [s for n, s in shapes.items() if pr.limit_case(n)[3][-1] == "radmin"]
    assert any("A" in s and len(s) < 20 for s in floor) and any(set(s) == {"C"} for s in floor) and any(set(s) == {"R"} for s in floor)
    # one workgroup, four fates: 0 iterations, an easy solve, the cap, the radius floor
    its = [int(pr.limit_case(n)[2]["iterations"][0]) for n in pr.FOUR_FATES]
    assert its[0] == 0 and 3 <= its[1] <= 4 and its[2] == 20 and its[3] < 20 and pr.limit_case(pr.FOUR_FATES[3])[3][-1] == "radmin", its
    ref = pr.frames(windows["four_fates_straddling"])
    assert list(ref["iterations"][3:]) == its and ref["status"] == pr.OK
    ref = pr.frames(windows["empty_between"])
    assert (ref["status"], ref["fail_frame"], ref["n_used"][1]) == (pr.FAIL_FEW_POINTS, 1, 0) and list(ref["iterations"][[0, 2]]) == its[1:3]
    assert len(windows["full_window"]["guess_key"]) == pr.MAX_FRAMES
