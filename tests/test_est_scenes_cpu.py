"""The scenes of tests/est_scenes.py are what tests/test_gpu_est_limits.py takes them for, checked with the restatement alone: every
state is one vio_est_state_set accepts, every slide case has the counts its name says, every update case takes the branch it is
named for (by tests/est_reference.py and by the 50-digit tests/est_exact.py, which also holds the restatement's double2vector to
UPDATE_TOL), and every scripted life fills its window, slides both ways, fires its one gate, and, where it is heavy, meets the pool
limit and is freed again."""
import numpy as np
import pytest

import est_exact
import est_reference as er
import est_scenes as sc

HEAVY_SEEDS = {sc.LIFE_SLOTS.index(s) for s in sc.LIFE_HEAVY}


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


@pytest.mark.parametrize("count", [63, 64, 65, 256])
def test_batch_states_are_valid_distinct_and_cover_every_frame_count(count):
    states = sc.batch_states(count)
    assert len(states) == count and all(sc.valid_state(s) for s in states)
    assert len({s["Ps"].tobytes() for s in states}) == count and len({s["Headers"].tobytes() for s in states}) == count
    assert [s["frame_count"] for s in states] == [k % 11 for k in range(count)]
    for s in states:
        n = np.diff(s["off"])
        assert n.max(initial=0) <= 5 and not n[s["frame_count"] + 1:].any()
    holes = [k for k, s in enumerate(states) if not s["exists"][:s["frame_count"] + 1].all()]
    assert len(holes) in (count // 11, count // 11 + 1) and all(int((1 - states[k]["exists"][:states[k]["frame_count"] + 1]).sum()) == 1 for k in holes)
    assert any(states[k]["frame_count"] == 10 for k in holes) == (count == 256)
    assert {s["failure_occur"] for s in states} == {0, 1} and any(int(s["off"][11]) == 0 for s in states)


def test_slide_cases_hold_what_their_names_say():
    cases = sc.slide_cases()
    assert [(d, t) for _, k, d, t, _ in cases if k == er.MARG_OLD] == sc.OLD_EDGES and len(cases) == len(sc.OLD_EDGES) + 2
    for name, kind, d, tail, counts in cases:
        s = sc.make_state(1, counts)
        assert sc.valid_state(s) and len(counts) == 11, name
        if kind == er.MARG_OLD:
            assert counts[0] == d and sum(counts[1:]) == tail and d + tail <= er.MAX_SAMPLES, name
            held = [j for j in range(1, 11) if counts[j]]
            assert tail == 0 or (len(held) >= 3 and any(counts[j] == 0 for j in range(held[0], held[-1]))), name     # spread, with empty ones between
            want, slid, _ = er.slide_window(s, kind)
            assert slid == 1 and int(want["off"][11]) == tail and np.array_equal(want["dt"], s["dt"][d:]), name
        else:
            assert sum(counts) == er.MAX_SAMPLES and counts[9] == 0, name
    news = [c for _, k, _, _, c in cases if k == er.MARG_SECOND_NEW]
    assert [c[10] > 0 for c in news] == [True, False]
    tails = [t for _, k, _, t, _ in cases if k == er.MARG_OLD]
    assert {sc.CHUNK, sc.CHUNK - 1, sc.CHUNK + 1, 2 * sc.CHUNK, 0, er.MAX_SAMPLES - 1} <= set(tails)


def old_cases():
    return [(name,) + sc.update_case(name) for name in sc.UPDATE_CASES]


def test_update_cases_take_their_branches_and_the_restatement_agrees_with_50_digits():
    """Every old and new update case: the branch by both references, the pitch values more than 1e-6 from the branch test, the gates
    as the case says, and est_reference.double2vector within UPDATE_TOL of est_exact.  The largest difference is printed."""
    worst = 0.0
    steps = []
    for name, s, win in old_cases():
        steps.append((name, s, win, int(name.startswith("singular")), 0))
    for c in sc.update_cases():
        s = c["state"]
        assert sc.valid_state(s), c["name"]
        for k, win in enumerate(c["steps"]):
            steps.append(("%s[%d]" % (c["name"], k), s, win, c["singular"][k], c["gate"][k]))
            s = er.double2vector(s, *win, True)[0]
    for name, s, (poses, sb, ext), singular, gate in steps:
        want, failure, gt, sing = er.double2vector(s, poses, sb, ext, True)
        ex = est_exact.double2vector(s, poses, sb)
        assert sing == ex["singular"] == singular, name
        assert (failure, gt) == (int(gate != 0), gate), name
        assert sc.branch_margin(s, poses) > 1e-6 and min(abs(abs(abs(p) - 90) - 1.0) for p in ex["pitch"]) > 1e-6, name
        for k in ("Rs", "Ps", "Vs"):
            err = rel(want[k], ex[k])
            worst = max(worst, err)
            assert err <= sc.UPDATE_TOL, (name, k, err)
        q = er.vector2double(want)[0][:, 3:7]
        err = rel(q, ex["quats"])
        worst = max(worst, err)
        assert err <= sc.UPDATE_TOL, (name, "quaternions", err)
    print("double2vector: restatement against 50 digits, largest relative difference %.3e over %d updates" % (worst, len(steps)))
    by = {c["name"]: c for c in sc.update_cases()}
    a = by["singular_by_last_R0"]                          # the pole is in last_R0 alone: Rs[0] and the solved frame are 50 degrees away
    assert a["state"]["failure_occur"] == 1
    assert abs(er.R2ypr(er.F(a["state"]["last_R0"]))[1] - 89.5) < 1e-9 and abs(er.R2ypr(er.F(a["state"]["Rs"][0]))[1] - 40.0) < 1e-9
    wrong = er.mul33(er.F(a["state"]["last_R0"]), er.transpose33(er.quat_to_rot(er.F(a["steps"][0][0][0, 3:7]))))
    right = er.mul33(er.F(a["state"]["Rs"][0]), er.transpose33(er.quat_to_rot(er.F(a["steps"][0][0][0, 3:7]))))
    assert np.abs(np.array(wrong) - np.array(right)).max() > 0.1      # (rot_diff from the wrong matrix is another rotation)
    b = by["pole_in_Rs0_only"]
    assert b["state"]["failure_occur"] == 1 and abs(er.R2ypr(er.F(b["state"]["Rs"][0]))[1] - 89.5) < 1e-9
    assert er.double2vector(dict(b["state"], failure_occur=0), *b["steps"][0], True)[3] == 1       # (through Rs[0] it would be singular)
    w = by["yaw_wrap"]
    ex = est_exact.double2vector(w["state"], *w["steps"][0][:2])
    assert abs(ex["y_diff"] - 358.0) < 1e-6
    g = by["gate_then_reanchor"]
    t1 = er.double2vector(g["state"], *g["steps"][0], True)[0]
    assert g["state"]["failure_occur"] == 0 and t1["failure_occur"] == 1 and np.array_equal(t1["last_P0"], g["state"]["last_P0"])
    t2 = er.double2vector(t1, *g["steps"][1], True)[0]
    assert np.abs(t2["Ps"][0] - g["state"]["last_P0"]).max() < 1e-12 and np.abs(t2["Ps"][0] - t1["Ps"][0]).max() > 1e-3
    plain = er.double2vector(dict(t1, failure_occur=0), *g["steps"][1], True)[0]
    assert np.abs(plain["Rs"] - t2["Rs"]).max() > 1e-3      # (anchoring on Rs[0] / Ps[0] instead gives another window)


def play(script, slot=0):
    """A life through the restatement: what happened, in the words the conditions below use."""
    ref, wins = sc.life_reference(), {}
    seen = dict(full=0, slides={er.MARG_OLD: 0, er.MARG_SECOND_NEW: 0}, gates=[], pool_full=0, freed=0, rounds=0, init=[], relin=0, zero_imu=0,
                stalls=0, missing_window=0, margin=np.inf)
    waiting = False
    for kind, args in script:
        before = ref.state_get(slot)
        if kind == "update":
            seen["margin"] = min(seen["margin"], sc.branch_margin(before, sc.life_solved(wins[slot], args)[0]))
        r = sc.issue(ref, kind, [(slot, args)], wins)[0]
        after = ref.state_get(slot)
        assert sc.valid_state(after)
        if kind == "imu":
            seen["zero_imu"] += int(before["frame_count"] == 0 and len(args[0]) > 0)
            if r["status"] == er.STATUS_POOL_FULL:
                seen["pool_full"] += 1
                waiting = True
            elif waiting and len(args[0]) > 0 and before["frame_count"] > 0:
                seen["freed"] += 1
                waiting = False
        if kind == "image":
            seen["stalls"] += int(not args[1] and before["frame_count"] < 10)
            seen["full"] += int(before["frame_count"] == 9 and after["frame_count"] == 10)
        if kind == "window":
            assert before["frame_count"] == 10
            seen["missing_window"] += int(not before["exists"][1:].all())
        if kind == "update":
            assert r["singular"] == 0
            if r["failure"]:
                seen["gates"].append(r["gate"])
        if kind == "slide":
            assert r["slid"] == 1
            seen["slides"][args[0]] += 1
            seen["rounds"] += 1
        if kind == "init_apply":
            seen["init"].append(r["status"])
        if kind == "relinearize":
            assert before["frame_count"] == 10
            seen["relin"] += r["n_relinearized"]
    return seen


@pytest.mark.parametrize("k", range(len(sc.LIFE_SLOTS)))
def test_a_life_is_what_the_lock_step_test_takes_it_for(k):
    kind = "heavy" if k in HEAVY_SEEDS else "normal"
    script = sc.life(k, kind)
    calls = [c for c, _ in script]
    assert calls[0] == "reset" and calls.count("reset") == 2 and calls[calls.index("reset", 1) - 1] == "update"      # as the drivers do
    first_image = calls.index("image")
    assert set(calls[1:first_image]) == {"imu"}                                   # IMU runs at frame_count 0 come first
    assert calls.count("image") >= 11 and calls.count("update") >= 25 and calls.count("init_apply") == 1 and calls.count("relinearize") >= 3
    lens = [len(a[0]) for c, a in script if c == "imu"]
    assert (set(lens) <= set(range(372, 401))) if kind == "heavy" else (set(lens) == set(sc.RUNS))
    seen = play(script)
    assert seen["full"] == 2 and seen["zero_imu"] >= 2 and seen["stalls"] >= 3
    assert seen["slides"][er.MARG_OLD] >= 5 and seen["slides"][er.MARG_SECOND_NEW] >= 3 and seen["rounds"] >= 20
    assert seen["gates"] == [er.GATE_BA] and seen["init"] == [0] and seen["relin"] >= 1 and seen["margin"] > 1e-6
    if kind == "heavy":
        assert seen["pool_full"] >= 1 and seen["freed"] >= 1
    print("life %d (%s): %d calls, %d samples, %d slides old / %d new, %d refused runs, %d windows with a missing interval"
          % (k, kind, len(script), sum(lens), seen["slides"][er.MARG_OLD], seen["slides"][er.MARG_SECOND_NEW], seen["pool_full"], seen["missing_window"]))


def test_lives_differ_and_normal_lives_leave_some_interval_unconstructed():
    scripts = [sc.life(k, "heavy" if k in HEAVY_SEEDS else "normal") for k in range(len(sc.LIFE_SLOTS))]
    assert len({tuple(c for c, _ in s) for s in scripts}) > 1
    assert any(play(s)["missing_window"] for k, s in enumerate(scripts) if k not in HEAVY_SEEDS)
