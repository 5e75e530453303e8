"""libvio_est_hip.so (include/vio_est.h, include/vio_est_init.h) at its limits, against tests/est_reference.py and
tests/est_init_reference.py through state_get: every batched call over 63, 64, 65 and 256 slots listed in a shuffled order (k_est_image
packs 64 items into a workgroup, and the uploads and vio_est_window_batch's 10 * count records are sized by count), the sample move
of k_est_slide at the edges of its chunks of 256 and on a full pool, IMU runs of 4096 samples and empty runs between others,
double2vector where failure_occur meets the singular branch, where the verdict itself raised the flag and where the yaw difference
wraps (against the restatement and against the 50-digit tests/est_exact.py), eight streams' scripted lives in lock-step with the
restatement, and reset / set_config / state_get at their rules.  The scenes are tests/est_scenes.py's; tests/test_est_scenes_cpu.py
checks on the CPU that they are what they are taken for.  Bit for bit everywhere but behind double2vector (UPDATE_TOL).  A missing
library is a failure, not a skip."""
import ctypes as C

import numpy as np
import pytest

import est_exact
import est_init_reference as eir
import est_reference as er
import est_scenes as sc
from est_scenes import G, NOISE, RIC_Q, TIC, UPDATE_TOL, make_state
from test_est_init_reference import T_A, T_G, init_inputs
from test_gpu_est import differing, eh, est_lib, imu_records, seed_slots, window_intervals  # noqa: F401  (two are fixtures)

pytestmark = pytest.mark.gpu

COUNTS = (63, 64, 65, 256)
RES_INTS = ("status", "frame_count", "n_samples", "failure", "gate", "singular", "slid", "shift_depth")
RES_ARRAYS = ("marg_R", "marg_P", "new_R", "new_P")
LOOSE = ("Rs", "Ps", "Vs", "last_R", "last_P", "last_R0", "last_P0")          # what double2vector's atan2 / sin / cos reach


@pytest.fixture(scope="module")
def states():
    return sc.batch_states(256)                             # (state k does not depend on the count: a batch is the first `count`)


def reference(states=(), slots=()):
    ref = eir.EstimatorInitReference()
    ref.set_config(TIC, RIC_Q, G, NOISE)
    for slot, s in zip(slots, states):
        ref.state_set(slot, s)
    return ref


def result_differs(got, want):
    """The fields of a batched call's result that are not the same bits."""
    bad = [k for k in RES_INTS if k in want and got[k] != want[k]]
    bad += [k for k in ("n_relinearized", "mask") if k in want and got[k] != want[k]]
    return bad + [k for k in RES_ARRAYS if k in want and np.asarray(got[k]).tobytes() != np.asarray(want[k], dtype=np.float64).tobytes()]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def loosely(got, want, where):
    """Two states behind an update: LOOSE within UPDATE_TOL, everything else the same bits.  Returns the largest difference."""
    worst = 0.0
    for k in LOOSE:
        err = rel(got[k], want[k])
        worst = max(worst, err)
        assert err <= UPDATE_TOL, (where, k, err)
    assert set(differing(got, want)) <= set(LOOSE), (where, differing(got, want))
    return worst


# ---- a. full batches --------------------------------------------------------------------------------------------------------------
def full_batch(eh, states, count, call):
    """Seeds slots 0 .. count - 1, makes `call` (of a handle and the shuffled slot list; returns the results) on the library and on
    the restatement and compares every result and every slot's state; at 65 also the 191 slots the call does not list."""
    slots = [int(x) for x in np.random.RandomState(count).permutation(count)]
    assert slots != sorted(slots)
    seed_slots(eh, states[:count], range(count))
    ref = reference(states[:count], range(count))
    rest = {s: eh.state_get(s) for s in range(count, er.MAX_SLOTS)} if count == 65 else {}
    got, want = call(eh, slots), call(ref, slots)
    assert len(got) == len(want) == count
    for slot, g, w in zip(slots, got, want):
        assert result_differs(g, w) == [], (count, slot)
    for s, before in rest.items():
        assert differing(eh.state_get(s), before) == [], (count, s)
    return slots, ref, got, want


def same_states(eh, ref, count):
    for slot in range(count):
        assert differing(eh.state_get(slot), ref.state_get(slot)) == [], (count, slot)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_image(eh, states, count):
    """A header of its own per item and alternating advance, against process_image; slots at frame_count 10 take the header and stay."""
    slots, ref, got, _ = full_batch(eh, states, count, lambda h, slots: h.image_batch([(s, 2000.0 + 0.125 * i, i % 2 == 0) for i, s in enumerate(slots)]))
    for i, (slot, r) in enumerate(zip(slots, got)):
        want = er.process_image(states[slot], 2000.0 + 0.125 * i, i % 2 == 0)
        assert r["frame_count"] == want["frame_count"] and differing(eh.state_get(slot), want) == [], (count, slot)
    assert sum(states[s]["frame_count"] == 10 for s in slots) >= 5
    same_states(eh, ref, count)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_imu(eh, states, count):
    rng = np.random.RandomState(count)
    runs = [sc.samples(rng, int(rng.randint(0, 6))) for _ in range(count)]
    assert sum(len(r[0]) == 0 for r in runs) >= 5
    slots, ref, _, _ = full_batch(eh, states, count, lambda h, slots: h.imu_batch([(s,) + r for s, r in zip(slots, runs)]))
    for slot, r in zip(slots, runs):
        assert differing(eh.state_get(slot), er.process_imu(states[slot], *r)[0]) == [], (count, slot)
    same_states(eh, ref, count)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_window(vio, eh, states, count):
    """vector2double bit for bit, and the 10 * count records byte for byte against libvio_imu_hip on one handle that holds every interval."""
    slots, ref, got, want = full_batch(eh, states, count, lambda h, slots: h.window_batch(slots))
    ivs, lbs = [], []
    for slot, g, w in zip(slots, got, want):
        for k in ("poses", "speed_bias", "ext"):
            assert g[k].tobytes() == w[k].tobytes(), (count, slot, k)
        iv, lb = window_intervals(states[slot])
        ivs += iv
        lbs.append(lb)
    recs = imu_records(vio, ivs, np.concatenate(lbs))
    assert len(recs) == 10 * count
    for i, (slot, g) in enumerate(zip(slots, got)):
        for j in range(10):
            assert bytes(g["preint"][j]) == recs[10 * i + j], (count, slot, j + 1)
    same_states(eh, ref, count)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_update(eh, states, count):
    rng = np.random.RandomState(count)
    wins = {slot: sc.solved_window(rng, states[slot], sc.ypr(float(rng.uniform(-170, 170)), 0.0, 0.0)) for slot in range(count)}
    assert all(sc.branch_margin(states[slot], wins[slot][0]) > 1e-6 for slot in range(count))
    slots, ref, got, want = full_batch(eh, states, count, lambda h, slots: h.update_batch([(s,) + wins[s] + (s % 2 == 0,) for s in slots]))
    assert {w["failure"] for w in want} == {0, 1}
    worst = 0.0
    for slot, g, w in zip(slots, got, want):
        worst = max(worst, loosely(eh.state_get(slot), ref.state_get(slot), (count, slot)))
        for k in ("poses", "speed_bias", "ext"):
            assert rel(g[k], w[k]) <= UPDATE_TOL, (count, slot, k)
    print("update_batch over %d slots: largest relative difference to the restatement %.3e" % (count, worst))


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_slide(eh, states, count):
    slots, ref, got, _ = full_batch(eh, states, count, lambda h, slots: h.slide_batch([(s, (s // 11) % 2, s % 3 != 0) for s in slots]))
    assert {(r["slid"], r["shift_depth"]) for r in got} == {(0, 0), (1, 0), (1, 1)}
    same_states(eh, ref, count)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_relinearize(eh, states, count):
    slots, ref, got, _ = full_batch(eh, states, count, lambda h, slots: h.relinearize_batch([(s, T_A * (1 + s % 3), T_G) for s in slots]))
    assert len({r["mask"] for r in got}) > 10 and any(r["mask"] == 0 for r in got)
    same_states(eh, ref, count)


@pytest.mark.parametrize("count", COUNTS)
def test_full_batch_init_apply(eh, states, count):
    ins = {slot: init_inputs(3000 + slot, 1.0003) + (slot % 2 == 1,) for slot in range(count)}
    slots, ref, got, _ = full_batch(eh, states, count, lambda h, slots: h.init_apply_batch([(s,) + ins[s] for s in slots]))
    ready = [s for s in slots if states[s]["frame_count"] == 10 and states[s]["exists"].all()]
    assert [s for s, r in zip(slots, got) if r["status"] == 0] == ready and len(ready) >= 5
    assert {r["status"] for r in got} == {0, eir.STATUS_NOT_READY}
    same_states(eh, ref, count)


# ---- b. slide at chunk edges --------------------------------------------------------------------------------------------------------
SLIDE_CASES = sc.slide_cases()


@pytest.mark.parametrize("name,kind,d,tail,counts", SLIDE_CASES, ids=[c[0] for c in SLIDE_CASES])
def test_slide_at_the_edges_of_a_chunk(vio, eh, name, kind, d, tail, counts):
    """Three slots in one call: the state bit for bit against slide_window, then the next window call's records byte for byte against
    libvio_imu_hip on the samples the restatement holds."""
    slots = (3, 64, 254)
    sts = [make_state(700 + 3 * len(name) + k, counts) for k in range(3)]
    seed_slots(eh, sts, slots)
    res = eh.slide_batch([(slot, kind, True) for slot in slots])
    wants = []
    for slot, s, r in zip(slots, sts, res):
        want, slid, mats = er.slide_window(s, kind)
        assert (r["slid"], slid, r["frame_count"], r["n_samples"]) == (1, 1, 10, int(want["off"][11])), (name, slot)
        assert r["n_samples"] == (tail if kind == er.MARG_OLD else er.MAX_SAMPLES)
        assert differing(eh.state_get(slot), want) == [], (name, slot)
        if mats is not None:
            for key, m in zip(RES_ARRAYS, mats):
                assert r[key].tobytes() == np.array(m).tobytes(), (name, key)
        wants.append(want)
    wins = eh.window_batch(list(slots))
    ivs, lbs = [], []
    for want in wants:
        iv, lb = window_intervals(want)
        ivs += iv
        lbs.append(lb)
    recs = imu_records(vio, ivs, np.concatenate(lbs))
    for i, (slot, w) in enumerate(zip(slots, wins)):
        for j in range(10):
            assert bytes(w["preint"][j]) == recs[10 * i + j], (name, slot, j + 1)


# ---- c. IMU runs --------------------------------------------------------------------------------------------------------------------
def test_a_run_of_4096_fills_an_empty_slot_and_one_more_sample_is_refused(eh):
    s = make_state(801, [0, 0], fc=1)
    run = sc.samples(np.random.RandomState(1), er.MAX_SAMPLES)
    seed_slots(eh, [s], [9])
    r = eh.imu_batch([(9,) + run])[0]
    want, st = er.process_imu(s, *run)
    assert (r["status"], st, r["n_samples"]) == (0, 0, er.MAX_SAMPLES)
    full = eh.state_get(9)
    assert differing(full, want) == [] and full["off"][11] == er.MAX_SAMPLES
    r = eh.imu_batch([(9,) + sc.samples(np.random.RandomState(2), 1)])[0]
    assert (r["status"], r["n_samples"]) == (er.STATUS_POOL_FULL, er.MAX_SAMPLES) and differing(eh.state_get(9), full) == []


def test_a_run_of_4096_at_frame_count_zero_stores_nothing(eh):
    s = make_state(802, [], fc=0)
    run = sc.samples(np.random.RandomState(3), er.MAX_SAMPLES)
    seed_slots(eh, [s], [250])
    r = eh.imu_batch([(250,) + run])[0]
    got = eh.state_get(250)
    assert (r["status"], r["n_samples"]) == (0, 0) and differing(got, er.process_imu(s, *run)[0]) == []
    assert got["off"][11] == 0 and np.array_equal(got["acc_0"], run[1][-1]) and np.array_equal(got["gyr_0"], run[2][-1])
    assert np.array_equal(got["Ps"], s["Ps"]) and np.array_equal(got["Rs"], s["Rs"])


def test_empty_runs_between_others_in_one_call(eh):
    """Runs of 4096, 0, 1, 0 and 65 samples in one call: the upload's offsets repeat where a run is empty."""
    lens, slots = (er.MAX_SAMPLES, 0, 1, 0, 65), (200, 5, 64, 63, 255)
    sts = [make_state(810, [0, 0, 0, 0], fc=3)] + [make_state(811 + k, [0, 3, 0, 5], fc=3 + k) for k in range(4)]
    rng = np.random.RandomState(4)
    runs = [sc.samples(rng, n) for n in lens]
    seed_slots(eh, sts, slots)
    res = eh.imu_batch([(slot,) + r for slot, r in zip(slots, runs)])
    for slot, s, run, r, n in zip(slots, sts, runs, res, lens):
        want, st = er.process_imu(s, *run)
        assert (r["status"], st, r["n_samples"]) == (0, 0, int(s["off"][11]) + n), slot
        assert differing(eh.state_get(slot), want) == [], (slot, n)


# ---- d. update ----------------------------------------------------------------------------------------------------------------------
def test_update_where_the_flag_meets_the_branches_against_the_restatement_and_50_digits(eh):
    """est_scenes.update_cases() on the device, one slot per case, the steps of a case one call after the other: results as the case
    says; the state within UPDATE_TOL of the restatement (run from the case's own state, so its second step starts from the
    restatement's first) and Rs / Ps / Vs and the returned quaternions within UPDATE_TOL of tests/est_exact.py.  Measured on an
    MI355X: 2.776e-16 against the restatement, 4.441e-16 against 50 digits (printed)."""
    cases = sc.update_cases()
    slots = (0, 7, 64, 255)
    seed_slots(eh, [c["state"] for c in cases], slots)
    refs = [c["state"] for c in cases]
    worst_r = worst_x = 0.0
    for k in range(max(len(c["steps"]) for c in cases)):
        live = [(slot, c, s) for slot, c, s in zip(slots, cases, refs) if k < len(c["steps"])]
        res = eh.update_batch([(slot,) + c["steps"][k] + (True,) for slot, c, _ in live])
        for (slot, c, s), r in zip(live, res):
            name = "%s[%d]" % (c["name"], k)
            poses, sb, ext = c["steps"][k]
            want, failure, gate, singular = er.double2vector(s, poses, sb, ext, True)
            assert (r["failure"], r["gate"], r["singular"]) == (failure, gate, singular) == (int(c["gate"][k] != 0), c["gate"][k], c["singular"][k]), name
            got = eh.state_get(slot)
            worst_r = max(worst_r, loosely(got, want, name))
            assert got["failure_occur"] == failure
            ex = est_exact.double2vector(s, poses, sb)
            assert ex["singular"] == singular, name
            for key in ("Rs", "Ps", "Vs"):
                err = rel(got[key], ex[key])
                worst_x = max(worst_x, err)
                assert err <= UPDATE_TOL, (name, key, err)
            err = rel(r["poses"][:, 3:7], ex["quats"])
            worst_x = max(worst_x, err)
            assert err <= UPDATE_TOL, (name, "quaternions", err)
            back = er.vector2double(got)
            assert r["poses"].tobytes() == back[0].tobytes() and r["speed_bias"].tobytes() == back[1].tobytes() and r["ext"].tobytes() == back[2].tobytes()
            refs[slots.index(slot)] = want
    print("update cases: largest relative difference to the restatement %.3e, to the 50-digit reference %.3e" % (worst_r, worst_x))
    by = {c["name"]: (eh.state_get(slot), c) for slot, c in zip(slots, cases)}
    got, c = by["singular_by_last_R0"]                      # rot_diff = Rs[0] R00^T undoes the gauge: the rotations come back, on last_P0
    assert rel(got["Rs"], c["state"]["Rs"]) < 1e-12 and rel(got["Ps"][0], c["state"]["last_P0"]) < 1e-12
    got, c = by["gate_then_reanchor"]
    assert rel(got["Ps"][0], c["state"]["last_P0"]) < 1e-12 and got["failure_occur"] == 0 and np.array_equal(got["last_P0"], got["Ps"][0])


def test_update_without_outputs_leaves_the_same_state(vio, eh):
    e = vio.est
    s, (poses, sb, ext) = sc.update_case("non_unit")
    seed_slots(eh, [s, s], (11, 12))
    with_out = eh.update_batch([(11, poses, sb, ext, True)])[0]
    item = (e.VioEstUpdateItem * 1)(e.VioEstUpdateItem(12, 1, poses.ctypes.data, sb.ctypes.data, ext.ctypes.data, None, None, None))
    res = (e.VioEstResult * 1)()
    assert eh.lib.fn["update_batch"](eh.h, C.c_int32(1), C.addressof(item), C.addressof(res)) == 0
    assert (res[0].failure, res[0].gate, res[0].singular, res[0].frame_count) == (with_out["failure"], with_out["gate"], with_out["singular"], 10)
    assert differing(eh.state_get(12), eh.state_get(11)) == [] and differing(eh.state_get(12), s) != []


# ---- e. a stream's life in lock-step ------------------------------------------------------------------------------------------------
def lock_step(h, ref, slots, scripts, check_all=True):
    """Every slot's script on the library and on the restatement, one batched call per step for the slots whose next call has the
    step's kind (the kind most slots wait for); after every step every slot's state and the call's results, bit for bit; behind an
    update within UPDATE_TOL, and then the restatement takes the device's state.  Returns what happened."""
    at = {slot: 0 for slot in slots}
    wins, ref_wins = {}, {}
    seen = dict(steps=0, pool_full=0, gates=0, slides={er.MARG_OLD: 0, er.MARG_SECOND_NEW: 0}, full=0, widest=0, worst=0.0, init=0, relin=0)
    while any(at[s] < len(scripts[s]) for s in slots):
        nxt = [scripts[s][at[s]][0] for s in slots if at[s] < len(scripts[s])]
        kind = max(sorted(set(nxt)), key=nxt.count)
        entries = [(s, scripts[s][at[s]][1]) for s in slots if at[s] < len(scripts[s]) and scripts[s][at[s]][0] == kind]
        got = sc.issue(h, kind, entries, wins)
        want = sc.issue(ref, kind, entries, wins if kind == "update" else ref_wins)     # (update: both take the device's window)
        for (slot, args), g, w in zip(entries, got, want):
            if kind == "reset":
                continue
            assert result_differs(g, w) == [], (seen["steps"], kind, slot, result_differs(g, w))
            if kind == "window":
                for k in ("poses", "speed_bias", "ext"):
                    assert g[k].tobytes() == w[k].tobytes(), (seen["steps"], slot, k)
                seen["full"] += 1
            if kind == "update":
                seen["worst"] = max(seen["worst"], loosely(h.state_get(slot), ref.state_get(slot), (seen["steps"], slot)))
                for k in ("poses", "speed_bias", "ext"):
                    assert rel(g[k], w[k]) <= UPDATE_TOL, (seen["steps"], slot, k)
                ref.state_set(slot, h.state_get(slot))
                seen["gates"] += g["failure"]
            if kind == "imu":
                seen["pool_full"] += int(g["status"] == er.STATUS_POOL_FULL)
            if kind == "slide":
                assert g["slid"] == 1
                seen["slides"][args[0]] += 1
            seen["init"] += int(kind == "init_apply" and g["status"] == 0)
            seen["relin"] += g["n_relinearized"] if kind == "relinearize" else 0
        for slot in (slots if check_all else [s for s, _ in entries]):
            assert differing(h.state_get(slot), ref.state_get(slot)) == [], (seen["steps"], kind, slot, differing(h.state_get(slot), ref.state_get(slot)))
        for slot, _ in entries:
            at[slot] += 1
        seen["steps"] += 1
        seen["widest"] = max(seen["widest"], len(entries))
    return seen


def test_eight_lives_in_lock_step_with_the_restatement(est_lib):
    h = est_lib.create()
    try:
        h.set_config(TIC, RIC_Q, sc.LIFE_G, NOISE)
        ref = sc.life_reference()
        scripts = {slot: sc.life(k, "heavy" if slot in sc.LIFE_HEAVY else "normal") for k, slot in enumerate(sc.LIFE_SLOTS)}
        seen = lock_step(h, ref, sc.LIFE_SLOTS, scripts)
        print("eight lives: %d steps for %d calls, at most %d slots in a call; %d windows, %d old and %d new slides, %d refused runs, %d gates; "
              "behind an update at most %.3e from the restatement" % (seen["steps"], sum(len(s) for s in scripts.values()), seen["widest"], seen["full"],
                                                                      seen["slides"][er.MARG_OLD], seen["slides"][er.MARG_SECOND_NEW], seen["pool_full"], seen["gates"], seen["worst"]))
        assert seen["gates"] == 8 and seen["init"] == 8 and seen["relin"] >= 8 and seen["pool_full"] >= 2 and seen["widest"] == 8
        assert seen["slides"][er.MARG_OLD] >= 8 * 15 and seen["slides"][er.MARG_SECOND_NEW] >= 8 * 3
        for slot in sc.LIFE_SLOTS:
            assert h.state_get(slot)["frame_count"] == 10
    finally:
        h.close()


# ---- f. reset, config, get ----------------------------------------------------------------------------------------------------------
def test_reset_of_a_slot_that_holds_samples_is_a_fresh_slot(eh):
    """A slot with 4095 samples is reset and lives a life's first steps beside a slot that was seeded empty with what clearState
    leaves alone, and beside the restatement."""
    used = make_state(901, [0] + [400] * 9 + [495])
    assert int(used["off"][11]) == er.MAX_SAMPLES - 1
    fresh = er.new_state(TIC, RIC_Q, G)
    for k in ("Headers", "acc_0", "gyr_0", "last_R", "last_P", "last_R0", "last_P0"):
        fresh[k] = used[k].copy()
    seed_slots(eh, [used, fresh], (6, 130))
    eh.reset(6)
    assert differing(eh.state_get(6), fresh) == [] and eh.state_get(6)["off"][11] == 0
    ref = reference([fresh], [130])
    script = [c for c in sc.life(3)[1:60] if c[0] in ("imu", "image")]
    assert sum(len(a[0]) for c, a in script if c == "imu") > 500 and sum(c == "image" for c, _ in script) >= 5
    wins = {}
    for kind, args in script:
        a, b = sc.issue(eh, kind, [(6, args), (130, args)], wins)
        w = sc.issue(ref, kind, [(130, args)], wins)[0]
        assert result_differs(a, b) == [] and result_differs(b, w) == []
    got = eh.state_get(6)
    assert differing(got, eh.state_get(130)) == [] and differing(got, ref.state_get(130)) == [] and got["off"][11] > 500 and got["frame_count"] >= 5


def test_set_config_changes_later_resets_only(est_lib):
    h = est_lib.create()
    try:
        one, two = ((0.1, 0.2, 0.3), (0.5, 0.5, -0.5, 0.5), (0.0, 0.1, 9.7)), ((-0.3, 0.0, 0.05), (0.0, 0.0, 0.6, 0.8), (0.2, 0.0, -9.8))
        default = er.new_state()
        assert differing(h.state_get(3), default) == []
        h.set_config(*one, NOISE)
        assert differing(h.state_get(3), default) == []     # set_config alone touches no slot
        h.reset(3)
        assert differing(h.state_get(3), er.new_state(*one)) == [] and differing(h.state_get(4), default) == []
        h.set_config(*two, NOISE)
        assert differing(h.state_get(3), er.new_state(*one)) == []      # a slot that is reset already keeps its own
        h.reset(4)
        assert differing(h.state_get(4), er.new_state(*two)) == [] and differing(h.state_get(3), er.new_state(*one)) == []
        h.reset(3)
        assert differing(h.state_get(3), er.new_state(*two)) == []
    finally:
        h.close()


def test_state_get_with_too_little_room_writes_the_offsets_only(vio, eh):
    e = vio.est
    s = make_state(902, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21])
    S = int(s["off"][11])
    seed_slots(eh, [s], [77])

    def raw(cap):
        st, off = e.VioEstState(), np.full(12, -1, dtype=np.int64)
        st.frame_count = -7
        dt, acc, gyr = np.full(S, np.nan), np.full((S, 3), np.nan), np.full((S, 3), np.nan)
        rc = eh.lib.fn["state_get"](eh.h, C.c_int32(77), C.addressof(st), C.c_int64(cap), off.ctypes.data, dt.ctypes.data, acc.ctypes.data, gyr.ctypes.data)
        return rc, st, off, dt, acc, gyr

    rc, st, off, dt, acc, gyr = raw(S - 1)
    assert rc == -1 and eh.last_error() and np.array_equal(off, s["off"])
    assert st.frame_count == -7 and np.isnan(dt).all() and np.isnan(acc).all() and np.isnan(gyr).all()      # nothing else is written
    assert differing(eh.state_get(77), s) == []
    rc, st, off, dt, acc, gyr = raw(S)
    assert rc == 0 and np.array_equal(off, s["off"]) and st.frame_count == 10
    assert dt.tobytes() == s["dt"].tobytes() and acc.tobytes() == s["acc"].tobytes() and gyr.tobytes() == s["gyr"].tobytes()


def test_the_callers_device_is_left_as_it_was(eh, states):
    import torch
    other = torch.cuda.device_count() >= 2
    if other:
        torch.cuda.set_device(1)
    cur = torch.cuda.current_device()
    try:
        slots = [0, 1, 2]
        seed_slots(eh, states[8:11], slots)
        run = sc.samples(np.random.RandomState(0), 3)
        calls = [lambda: eh.imu_batch([(s,) + run for s in slots]), lambda: eh.image_batch([(s, 1.0, True) for s in slots]), lambda: eh.window_batch(slots),
                 lambda: eh.update_batch([(s,) + sc.solved_window(np.random.RandomState(s), states[8 + s], sc.ypr(20.0, 0.0, 0.0)) + (True,) for s in slots]),
                 lambda: eh.slide_batch([(s, er.MARG_OLD, True) for s in slots]), lambda: eh.relinearize_batch([(s, T_A, T_G) for s in slots]),
                 lambda: eh.init_apply_batch([(s,) + init_inputs(s) for s in slots]), lambda: eh.reset(1), lambda: eh.state_get(2)]
        for k, call in enumerate(calls):
            call()
            assert torch.cuda.current_device() == cur, k
    finally:
        if other:
            torch.cuda.set_device(0)
