"""The batched Estimator state on the GPU (csrc/libvio_est_hip.so, include/vio_est.h) against tests/est_reference.py: processIMU,
vector2double and slideWindow bit for bit, the window's pre-integrations byte for byte against libvio_imu_hip (the same kernel text)
and within its tolerances of the host's vio_preintegrate, double2vector to 1e-12 (the device's atan2 / sin / cos), the gates of
failureDetection at their thresholds, the pool limit, independence of batch and slot index, and the argument errors.  A missing
library is a failure, not a skip."""
import ctypes as C

import numpy as np
import pytest

import est_reference as er
from est_scenes import G, NOISE, RIC_Q, TIC, UPDATE_CASES, UPDATE_TOL, make_state, rot, samples, solved_window, update_case, ypr  # noqa: F401  (the builders live there)

pytestmark = pytest.mark.gpu

SLOTS = (0, 7, 255)
VEC_TOL, BLOCK_TOL = 1e-13, 1e-12       # tests/test_gpu_imu.py's


@pytest.fixture(scope="module")
def est_lib(vio, hip_lib):
    return vio.load_est()


@pytest.fixture(scope="module")
def eh(est_lib):
    h = est_lib.create()
    h.set_config(TIC, RIC_Q, G, NOISE)
    yield h
    h.close()


FIELDS = list(er.new_state().keys())


def differing(got, want):
    """The fields of two states that are not the same bytes."""
    bad = []
    for k in FIELDS:
        a, b = got[k], want[k]
        if isinstance(b, np.ndarray):
            a, b = np.asarray(a, dtype=b.dtype).reshape(-1), b.reshape(-1)
            if a.shape != b.shape or a.tobytes() != b.tobytes():
                bad.append(k)
        elif int(a) != int(b):
            bad.append(k)
    return bad


def seed_slots(eh, states, slots=SLOTS):
    for slot, s in zip(slots, states):
        eh.state_set(slot, s)


# ---- 1. imu_batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_imu_batch_is_the_restatement_bit_for_bit(eh, n):
    states = [make_state(10 + k, [0, 3, 0, 5], fc=3 + k) for k in range(3)]
    seed_slots(eh, states)
    rng = np.random.RandomState(n)
    runs = [samples(rng, n) for _ in SLOTS]
    res = eh.imu_batch([(slot,) + r for slot, r in zip(SLOTS, runs)])
    for slot, s, r, out in zip(SLOTS, states, runs, res):
        want, st = er.process_imu(s, *r)
        assert (out["status"], out["frame_count"], out["n_samples"]) == (st, s["frame_count"], 8 + n)
        assert differing(eh.state_get(slot), want) == [], (slot, n)


def test_imu_runs_split_over_calls_equal_one_call(eh):
    s = make_state(21, [0, 2, 4], fc=2)
    dt, acc, gyr = samples(np.random.RandomState(3), 65)
    seed_slots(eh, [s, s, s])
    eh.imu_batch([(0, dt, acc, gyr)])
    for a, b in ((0, 1), (1, 64), (64, 64), (64, 65)):          # slot 7: 1 + 63 + 0 + 1; slot 255: the same cuts, other calls
        eh.imu_batch([(7, dt[a:b], acc[a:b], gyr[a:b])])
    eh.imu_batch([(255, dt[:33], acc[:33], gyr[:33])])
    eh.imu_batch([(255, dt[33:], acc[33:], gyr[33:])])
    want, _ = er.process_imu(s, dt, acc, gyr)
    for slot in SLOTS:
        assert differing(eh.state_get(slot), want) == [], slot


def test_imu_first_sample_and_frame_count_zero(eh):
    """frame_count == 0: interval 0 is constructed, nothing is pushed or propagated, acc_0 / gyr_0 move to the last sample.  The first
    sample ever sets acc_0 / gyr_0 before the interval is constructed from them."""
    for slot in SLOTS:
        eh.reset(slot)
    fresh = er.new_state(TIC, RIC_Q, G)
    assert differing(eh.state_get(7), dict(fresh, Headers=eh.state_get(7)["Headers"], acc_0=eh.state_get(7)["acc_0"], gyr_0=eh.state_get(7)["gyr_0"],
                                           last_R=eh.state_get(7)["last_R"], last_P=eh.state_get(7)["last_P"], last_R0=eh.state_get(7)["last_R0"],
                                           last_P0=eh.state_get(7)["last_P0"])) == []
    first = make_state(31, [0, 4], fc=1)
    first.update(first_imu=0)
    first["exists"][1] = 0
    first["first"][1], first["lin_bias"][1] = 0.0, 0.0
    first["off"], first["dt"], first["acc"], first["gyr"] = np.zeros(12, dtype=np.int64), np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))
    zero = dict(make_state(32, [], fc=0), first_imu=1)
    zero["exists"][0] = 0
    states = [zero, first, dict(zero, first_imu=0)]
    seed_slots(eh, states)
    runs = [samples(np.random.RandomState(40 + k), 5) for k in range(3)]
    eh.imu_batch([(slot,) + r for slot, r in zip(SLOTS, runs)])
    for slot, s, r in zip(SLOTS, states, runs):
        want, _ = er.process_imu(s, *r)
        got = eh.state_get(slot)
        assert differing(got, want) == [], slot
        assert np.array_equal(got["acc_0"], r[1][-1]) and got["first_imu"] == 1
    z = eh.state_get(0)
    assert z["off"][11] == 0 and z["exists"][0] == 1 and np.array_equal(z["Ps"], zero["Ps"]) and np.array_equal(z["first"][0, 0:3], zero["acc_0"])
    f = eh.state_get(7)
    assert np.array_equal(f["first"][1, 0:3], runs[1][1][0]) and f["off"][11] == 5 and not np.array_equal(f["Rs"][1], first["Rs"][1])


# ---- 2. the pool ------------------------------------------------------------------------------------------------------------------
def test_pool_limit_refuses_the_slot_and_leaves_it(eh):
    full = [0, 400, 400, 400, 400, 400, 400, 400, 400, 400, 495]
    assert sum(full) == er.MAX_SAMPLES - 1
    states = [make_state(51, full), make_state(52, full), make_state(53, [0, 2])]
    seed_slots(eh, states)
    before = eh.state_get(7)
    rng = np.random.RandomState(5)
    runs = [samples(rng, 1), samples(rng, 2), samples(rng, 2)]
    res = eh.imu_batch([(slot,) + r for slot, r in zip(SLOTS, runs)])
    assert [r["status"] for r in res] == [er.STATUS_OK, er.STATUS_POOL_FULL, er.STATUS_OK]
    assert [r["n_samples"] for r in res] == [er.MAX_SAMPLES, er.MAX_SAMPLES - 1, 4]
    assert differing(eh.state_get(7), before) == [] and differing(before, states[1]) == []
    for slot, s, r in ((0, states[0], runs[0]), (255, states[2], runs[2])):
        assert differing(eh.state_get(slot), er.process_imu(s, *r)[0]) == [], slot
    assert eh.imu_batch([(0,) + samples(rng, 1)])[0]["status"] == er.STATUS_POOL_FULL


# ---- 3. window_batch ---------------------------------------------------------------------------------------------------------------
def vec(p):
    return np.frombuffer(p, dtype=np.float64)


def check_close(got, ref, where=""):
    """tests/test_gpu_imu.py's comparison of two records."""
    g, r = vec(got), vec(ref)
    for name, a, b in (("sum_dt", 0, 1), ("delta_p", 1, 4), ("delta_q", 4, 8), ("delta_v", 8, 11)):
        scale = max(np.abs(r[a:b]).max(), 1e-300)
        assert np.abs(g[a:b] - r[a:b]).max() / scale <= VEC_TOL, (where, name)
    assert np.array_equal(g[11:17], r[11:17]), where
    for name, o in (("jacobian", 17), ("covariance", 242)):
        Gm, Rm = g[o:o + 225].reshape(15, 15), r[o:o + 225].reshape(15, 15)
        for bi in range(5):
            for bj in range(5):
                gb, rb = Gm[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3], Rm[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3]
                assert np.abs(gb - rb).max() <= BLOCK_TOL * np.abs(rb).max(), (where, name, bi, bj)


def window_intervals(s):
    """Intervals 1 .. 10 of a state as libvio_imu_hip's dicts, and their construction biases."""
    ivs = [er.interval_samples(s, j) for j in range(1, 11)]
    lb = np.array([s["lin_bias"][j] if s["exists"][j] else np.zeros(6) for j in range(1, 11)])
    return [dict(iv, dt=list(iv["dt"]), acc=list(iv["acc"]), gyr=list(iv["gyr"])) for iv in ivs], lb


def imu_records(vio, ivs, lb):
    ih = vio.load_imu().create()
    ih.load(ivs, NOISE)
    recs = ih.propagate(lb[:, 0:3], lb[:, 3:6])
    out = [bytes(r) for r in recs]
    ih.close()
    return out


def test_window_batch_states_and_preintegrations(vio, hip_lib, eh):
    """Interval 4 exists and is empty, interval 6 does not exist; 65 and 200 samples cross a wavefront's worth of lanes."""
    states = [make_state(61 + k, [0, 3, 20, 1, 0, 7, 0, 65, 2, 200, 20 + k], missing=(6,)) for k in range(3)]
    seed_slots(eh, states)
    res = eh.window_batch(list(SLOTS))
    empty = np.zeros(467)
    empty[7] = 1.0
    empty[17:242] = np.eye(15).reshape(-1)
    for slot, s, r in zip(SLOTS, states, res):
        poses, sb, ext = er.vector2double(s)
        assert r["poses"].tobytes() == poses.tobytes() and r["speed_bias"].tobytes() == sb.tobytes() and r["ext"].tobytes() == ext.tobytes(), slot
        assert {er.rot_to_quat(er.F(s["Rs"][i]))[1] for i in range(11)} == {0, 1, 2, 3}
        ivs, lb = window_intervals(s)
        same_kernel = imu_records(vio, ivs, lb)
        for j in range(10):
            got = bytes(r["preint"][j])
            assert got == same_kernel[j], (slot, j)
            host = hip_lib.preintegrate(ivs[j]["acc0"], ivs[j]["gyr0"], lb[j, 0:3].copy(), lb[j, 3:6].copy(), np.array(ivs[j]["dt"]).reshape(-1),
                                        np.array(ivs[j]["acc"]).reshape(-1, 3), np.array(ivs[j]["gyr"]).reshape(-1, 3), *[NOISE[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")])
            check_close(r["preint"][j], host, "slot %d interval %d" % (slot, j + 1))
        for j, bias in ((3, s["lin_bias"][4]), (5, np.zeros(6))):          # interval 4: empty; interval 6: missing
            want = empty.copy()
            want[11:17] = bias
            assert vec(r["preint"][j]).tobytes() == want.tobytes(), (slot, j)
        assert differing(eh.state_get(slot), s) == []


# ---- 4. update_batch ---------------------------------------------------------------------------------------------------------------
def test_update_batch_against_the_restatement(eh):
    """double2vector: Rs / Ps / Vs and last_* within 1e-12 of max(1, |array|) (device atan2 / sin / cos through two 3 x 3 products);
    Bas / Bgs / tic / ric bit for bit.  The measured maximum is printed (DESIGN.md section 30 records it)."""
    worst = 0.0
    for a in range(0, len(UPDATE_CASES), 3):
        names = UPDATE_CASES[a:a + 3]
        cases = [update_case(n) for n in names]
        seed_slots(eh, [c[0] for c in cases])
        res = eh.update_batch([(slot,) + c[1] + (True,) for slot, c in zip(SLOTS, cases)])
        for slot, name, (s, (poses, sb, ext)), r in zip(SLOTS, names, cases, res):
            want, failure, gate, singular = er.double2vector(s, poses, sb, ext, True)
            o, o0 = er.R2ypr(er.F(s["last_R0"] if s["failure_occur"] else s["Rs"][0])), er.R2ypr(er.quat_to_rot(er.F(poses[0, 3:7])))
            for pitch in (o[1], o0[1]):
                assert abs(abs(abs(pitch) - 90) - 1.0) > 1e-6      # (well away from the branch test)
            assert singular == int(name.startswith("singular")), name
            assert (r["failure"], r["gate"], r["singular"]) == (failure, gate, singular) == (0, 0, singular), name
            got = eh.state_get(slot)
            for k in ("Rs", "Ps", "Vs", "last_R", "last_P", "last_R0", "last_P0"):
                err = np.abs(got[k] - want[k]).max() / max(1.0, np.abs(want[k]).max())
                worst = max(worst, err)
                assert err <= UPDATE_TOL, (name, k, err)
            for k in ("Bas", "Bgs", "tic", "ric"):
                assert got[k].tobytes() == want[k].tobytes(), (name, k)
            assert set(differing(got, want)) <= {"Rs", "Ps", "Vs", "last_R", "last_P", "last_R0", "last_P0"}, name
            assert got["failure_occur"] == 0
            back = er.vector2double(got)                    # the call's outputs: vector2double of the state it left, bit for bit
            assert r["poses"].tobytes() == back[0].tobytes() and r["speed_bias"].tobytes() == back[1].tobytes() and r["ext"].tobytes() == back[2].tobytes()
            for a, b in zip(back, er.vector2double(want)):
                assert np.abs(a - b).max() / max(1.0, np.abs(b).max()) <= UPDATE_TOL, name
            if name == "failure_occur":                     # the gauge comes from last_R0 / last_P0, not from Rs[0] / Ps[0]
                assert np.abs(got["Ps"][0] - s["last_P0"]).max() < 1e-12 and np.abs(got["Ps"][0] - s["Ps"][0]).max() > 1e-3
            if name == "yaw_only":                          # the solve's yaw drift is undone
                assert np.abs(got["Rs"] - s["Rs"]).max() < 1e-12
    print("update_batch: largest relative difference to the restatement %.3e" % worst)


# ---- 5. the gates -------------------------------------------------------------------------------------------------------------------
def gate_case(Ba=(0, 0, 0), Bg=(0, 0, 0), P=(0, 0, 0), last_P=(0, 0, 0)):
    """A state and a solved window whose re-anchoring is exact: Rs[0] = I and Ps[0] = 0 before and after, so rot_diff is the identity
    (cos 0 = 1, sin 0 = 0) and Ps[10] is the solved position, Bas[10] / Bgs[10] are copies."""
    s = make_state(80, [0, 1])
    s["Rs"][0], s["Ps"][0] = np.eye(3).reshape(9), 0.0
    s["last_P"] = np.array(last_P, dtype=np.float64)
    poses, sb, ext = er.vector2double(s)
    poses[10, 0:3], sb[10, 3:6], sb[10, 6:9] = P, Ba, Bg
    return s, (poses, sb, ext)


up = np.nextafter
GATES = [(dict(Ba=(1.5, 2.0, 0)), 0), (dict(Ba=(2.5, 0, 0)), 0), (dict(Ba=(1.5, up(2.0, 3), 0)), 1), (dict(Ba=(up(2.5, 3), 0, 0)), 1),
         (dict(Bg=(1.0, 0, 0)), 0), (dict(Bg=(up(1.0, 2), 0, 0)), 2),
         (dict(P=(1 + 5 - 1e-9, 2, 0.5), last_P=(1, 2, 0.5)), 0), (dict(P=(1 + 5 + 1e-9, 2, 0.5), last_P=(1, 2, 0.5)), 3),
         (dict(P=(1, 2, 0.5 + 1 - 1e-9), last_P=(1, 2, 0.5)), 0), (dict(P=(1, 2, 0.5 - 1 - 1e-9), last_P=(1, 2, 0.5)), 4),
         (dict(Ba=(3, 0, 0), Bg=(2, 0, 0), P=(9, 9, 9)), 1), (dict(Bg=(2, 0, 0), P=(9, 9, 9)), 2), (dict(P=(9, 9, 9)), 3), (dict(P=(0, 0.5, 2)), 4)]


def test_gates_at_their_thresholds_and_commit_last(eh):
    for a in range(0, len(GATES), 3):
        group = GATES[a:a + 3]
        cases = [gate_case(**kw) for kw, _ in group]
        for commit in (True, False):
            seed_slots(eh, [c[0] for c in cases])
            res = eh.update_batch([(slot,) + c[1] + (commit,) for slot, c in zip(SLOTS, cases)])
            for slot, (kw, gate), (s, (poses, sb, ext)), r in zip(SLOTS, group, cases, res):
                assert er.double2vector(s, poses, sb, ext, commit)[1:3] == (int(gate != 0), gate), kw
                assert (r["failure"], r["gate"]) == (int(gate != 0), gate), kw
                got = eh.state_get(slot)
                assert got["failure_occur"] == int(gate != 0)
                assert np.array_equal(got["Ps"][10], poses[10, 0:3]) and np.array_equal(got["Bas"][10], sb[10, 3:6])
                committed = gate == 0 and commit                # :234-237 only without a failure, and only when asked
                assert np.array_equal(got["last_P"], got["Ps"][10] if committed else s["last_P"]), (kw, commit)
                assert np.array_equal(got["last_R0"], got["Rs"][0] if committed else s["last_R0"]), (kw, commit)
                assert np.array_equal(got["last_R"], got["Rs"][10] if committed else s["last_R"]) and \
                    np.array_equal(got["last_P0"], got["Ps"][0] if committed else s["last_P0"])


# ---- 6. slide_batch ----------------------------------------------------------------------------------------------------------------
SLIDES = [("old", er.MARG_OLD, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21], 10), ("new", er.MARG_SECOND_NEW, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21], 10),
          ("old_short", er.MARG_OLD, [0, 3, 20, 1], 9), ("new_short", er.MARG_SECOND_NEW, [0, 3, 20, 1], 3),
          ("new_empty_newest", er.MARG_SECOND_NEW, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 0], 10),
          ("old_drops_0", er.MARG_OLD, [0, 0, 20, 1, 0, 7, 0, 65, 2, 30, 21], 10), ("old_drops_1", er.MARG_OLD, [1, 3, 300, 1, 0, 7, 0, 65, 2, 30, 21], 10),
          ("old_drops_1025", er.MARG_OLD, [1025, 3, 300, 1, 0, 7, 0, 65, 2, 600, 21], 10)]


@pytest.mark.parametrize("name,kind,counts,fc", SLIDES, ids=[c[0] for c in SLIDES])
def test_slide_batch_is_the_restatement_bit_for_bit(eh, name, kind, counts, fc):
    """Old and new on a full window, both below it (a no-op that is reported), new with an empty newest interval, old where the dropped
    interval (interval 0: after the first slide it holds what was interval 1) has 0, 1 and 1025 samples; the last moves 2000 samples
    down in chunks of a workgroup."""
    states = [make_state(90 + k, counts, fc=fc) for k in range(3)]
    seed_slots(eh, states)
    res = eh.slide_batch([(slot, kind, k != 1) for k, slot in enumerate(SLOTS)])
    for k, (slot, s, r) in enumerate(zip(SLOTS, states, res)):
        want, slid, mats = er.slide_window(s, kind)
        assert (r["slid"], r["frame_count"], r["n_samples"]) == (slid, fc, int(want["off"][11])) and slid == int(fc == 10), name
        assert differing(eh.state_get(slot), want) == [], (name, slot)
        if mats is None:
            assert not r["marg_R"].any() and not r["new_P"].any() and r["shift_depth"] == 0
        else:
            assert r["shift_depth"] == int(k != 1)
            for key, m in zip(("marg_R", "marg_P", "new_R", "new_P"), mats):
                assert r[key].tobytes() == np.array(m).tobytes(), (name, key)


def test_two_old_slides_in_a_row(eh):
    """A window as the reference first fills it (interval 0 empty), slid twice: the second slide drops what was interval 1, with 0, 1
    and 1025 samples."""
    for k, n1 in enumerate((0, 1, 1025)):
        states = [make_state(95 + k, [0, n1, 300, 1, 0, 7, 0, 65, 2, 600 + j, 21]) for j in range(3)]
        seed_slots(eh, states)
        res = eh.slide_batch([(slot, er.MARG_OLD, True) for slot in SLOTS])
        for slot, s, r in zip(SLOTS, states, res):
            want, slid, _ = er.slide_window(s, er.MARG_OLD)
            assert slid == 1 and r["slid"] == 1
            assert differing(eh.state_get(slot), want) == [], (n1, slot)
        eh.slide_batch([(slot, er.MARG_OLD, True) for slot in SLOTS])          # a second slide drops the old interval 1: n1 samples
        for slot, s in zip(SLOTS, states):
            want2 = er.slide_window(er.slide_window(s, er.MARG_OLD)[0], er.MARG_OLD)[0]
            got = eh.state_get(slot)
            assert differing(got, want2) == [] and got["off"][11] == s["off"][11] - n1, (n1, slot)


def test_slide_matrices_are_the_stream_drivers(vio, eh):
    """marg_R, marg_P, new_R, new_P against StreamDriver.slide_window_old's formulas (stream.py:753-755) in numpy's matmul, from the
    same matrices: Rs[i] = synth.quat_to_rot(q_i) on both sides, |P| <= 1, so the only difference is the order of a three-term sum
    (a few 2^-53).  1e-15 absolute."""
    rng = np.random.RandomState(7)
    states, want = [], []
    for k in range(3):
        s = make_state(100 + k, [0, 2, 3])
        poses = np.zeros((11, 7))
        for i in range(11):
            q = vio.synth.rot_to_quat(ypr(*rng.uniform(-80, 80, 3)))
            poses[i, 0:3], poses[i, 3:7] = rng.uniform(-1, 1, 3), q
            s["Rs"][i], s["Ps"][i] = vio.synth.quat_to_rot(q).reshape(9), poses[i, 0:3]
        ext = np.concatenate([TIC, np.array(RIC_Q)])
        s["ric"] = vio.synth.quat_to_rot(ext[3:7]).reshape(9)
        R0, R1 = vio.synth.quat_to_rot(poses[0, 3:7]), vio.synth.quat_to_rot(poses[1, 3:7])
        ric, tic = vio.synth.quat_to_rot(ext[3:7]), ext[0:3]
        want.append((R0 @ ric, poses[0, 0:3] + R0 @ tic, R1 @ ric, poses[1, 0:3] + R1 @ tic))
        states.append(s)
    seed_slots(eh, states)
    res = eh.slide_batch([(slot, er.MARG_OLD, True) for slot in SLOTS])
    worst = 0.0
    for r, w in zip(res, want):
        for key, m in zip(("marg_R", "marg_P", "new_R", "new_P"), w):
            worst = max(worst, np.abs(r[key] - m).max())
    print("slide matrices: largest difference to numpy's %.3e" % worst)
    assert worst <= 1e-15


def test_merged_interval_is_one_preintegration_over_both(vio, eh):
    states = [make_state(110 + k, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30 + k, 21]) for k in range(3)]
    seed_slots(eh, states)
    eh.slide_batch([(slot, er.MARG_SECOND_NEW, True) for slot in SLOTS])
    res = eh.window_batch(list(SLOTS))
    for slot, s, r in zip(SLOTS, states, res):
        a, b = int(s["off"][9]), int(s["off"][11])
        both = dict(acc0=s["first"][9, 0:3], gyr0=s["first"][9, 3:6], dt=list(s["dt"][a:b]), acc=list(s["acc"][a:b]), gyr=list(s["gyr"][a:b]))
        assert b - a == 30 + SLOTS.index(slot) + 21
        assert bytes(r["preint"][8]) == imu_records(vio, [both], s["lin_bias"][9:10])[0], slot
        assert vec(r["preint"][9])[0] == 0.0 and np.array_equal(vec(r["preint"][9])[11:17], np.concatenate([s["Bas"][10], s["Bgs"][10]]))


# ---- 7. independence ---------------------------------------------------------------------------------------------------------------
def sequence(eh, slots, states, seed=0):
    """A fixed sequence of every call on `slots`; returns each slot's bytes: the state after it and the window in the middle."""
    rng = np.random.RandomState(seed)
    seed_slots(eh, states, slots)
    run1, run2 = samples(rng, 7), samples(rng, 70)
    eh.imu_batch([(slot,) + run1 for slot in slots])
    eh.image_batch([(slot, 123.5, True) for slot in slots])
    wins = eh.window_batch(list(slots))
    eh.update_batch([(slot, w["poses"], w["speed_bias"], w["ext"], True) for slot, w in zip(slots, wins)])
    r1 = eh.slide_batch([(slot, er.MARG_OLD, True) for slot in slots])
    eh.imu_batch([(slot,) + run2 for slot in slots])
    r2 = eh.slide_batch([(slot, er.MARG_SECOND_NEW, True) for slot in slots])
    out = []
    for i, slot in enumerate(slots):
        g = eh.state_get(slot)
        blob = b"".join(np.ascontiguousarray(g[k]).tobytes() for k in FIELDS if isinstance(g[k], np.ndarray))
        blob += bytes([g["frame_count"], g["first_imu"], g["failure_occur"]]) + b"".join(bytes(p) for p in wins[i]["preint"])
        blob += wins[i]["poses"].tobytes() + r1[i]["marg_R"].tobytes() + r1[i]["new_P"].tobytes() + bytes([r1[i]["slid"], r2[i]["slid"]])
        out.append(blob)
    return out


def test_a_slots_bytes_depend_neither_on_the_batch_nor_on_the_slot(eh):
    s = make_state(120, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21])
    others = [make_state(121, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]), make_state(122, [0, 400, 1], fc=2)]
    alone = sequence(eh, [5], [s])[0]
    assert sequence(eh, [5], [s])[0] == alone                                   # repeated: bitwise identical
    batch = sequence(eh, [9, 5, 200], [others[0], s, others[1]])
    assert batch[1] == alone and batch[0] != alone
    assert sequence(eh, [77], [s])[0] == alone                                  # another slot index
    assert sequence(eh, [200, 9, 5], [others[1], others[0], s]) == [batch[2], batch[0], alone]


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(vio, eh):
    e = vio.est
    states = [make_state(130 + k, [0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21]) for k in range(3)]
    seed_slots(eh, states)
    dt, acc, gyr = samples(np.random.RandomState(1), 4)
    poses, sb, ext = er.vector2double(states[0])
    bad_acc, bad_pose, bad_dt = acc.copy(), poses.copy(), dt.copy()
    bad_acc[2, 1], bad_pose[4, 5], bad_dt[3] = np.nan, np.inf, np.nan
    res = (e.VioEstResult * 4)()

    def raw(name, items):
        return eh.lib.fn[name](eh.h, C.c_int32(len(items)), C.addressof(items), C.addressof(res))

    null_item = (e.VioEstImuItem * 2)(e.VioEstImuItem(0, 4, dt.ctypes.data, acc.ctypes.data, gyr.ctypes.data), e.VioEstImuItem(7, 4, dt.ctypes.data, None, gyr.ctypes.data))
    neg_item = (e.VioEstImuItem * 2)(e.VioEstImuItem(0, 4, dt.ctypes.data, acc.ctypes.data, gyr.ctypes.data), e.VioEstImuItem(7, -1, dt.ctypes.data, acc.ctypes.data, gyr.ctypes.data))
    null_win = (e.VioEstUpdateItem * 1)(e.VioEstUpdateItem(0, 1, poses.ctypes.data, None, ext.ctypes.data, None, None, None))
    calls = [lambda: eh.imu_batch([(0, dt, acc, gyr), (256, dt, acc, gyr)]), lambda: eh.imu_batch([(0, dt, acc, gyr), (-1, dt, acc, gyr)]),
             lambda: eh.imu_batch([(0, dt, acc, gyr), (7, dt, acc, gyr), (0, dt, acc, gyr)]),
             lambda: eh.imu_batch([(0, dt, acc, gyr), (7, dt, bad_acc, gyr)]), lambda: eh.imu_batch([(0, dt, acc, gyr), (7, bad_dt, acc, gyr)]),
             lambda: eh.update_batch([(0, poses, sb, ext, True), (7, bad_pose, sb, ext, True)]),
             lambda: eh.update_batch([(0, poses, sb, ext, True), (0, poses, sb, ext, True)]),
             lambda: eh.slide_batch([(0, er.MARG_OLD, True), (7, 2, True)]), lambda: eh.slide_batch([(0, er.MARG_OLD, True), (300, er.MARG_OLD, True)]),
             lambda: eh.image_batch([(0, 1.0, True), (7, float("nan"), True)]), lambda: eh.window_batch([0, 7, 7]),
             lambda: eh.state_set(7, dict(states[1], frame_count=11)), lambda: eh.state_set(7, dict(states[1], Ps=np.full((11, 3), np.nan))),
             lambda: eh.state_set(7, dict(make_state(1, [0, 3, 20, 1], fc=3), frame_count=2))]
    for k, call in enumerate(calls):
        with pytest.raises(vio.VioError) as exc:
            call()
        assert exc.value.status == -1, k
        assert eh.last_error(), k
    for name, items in (("imu_batch", null_item), ("imu_batch", neg_item), ("update_batch", null_win)):
        assert raw(name, items) == -1 and eh.last_error()
    assert eh.lib.fn["imu_batch"](eh.h, C.c_int32(1), None, C.addressof(res)) == -1
    assert eh.lib.fn["imu_batch"](eh.h, C.c_int32(257), C.addressof(null_item), C.addressof(res)) == -1
    for slot, s in zip(SLOTS, states):
        assert differing(eh.state_get(slot), s) == [], slot
    assert eh.imu_batch([]) == [] and eh.window_batch([]) == []


# ---- 9. StreamDriver(state=) ---------------------------------------------------------------------------------------------------------
def run_streams(vio, hip_lib, make_handle, seeds=(0, 1, 2), nonkey_every=4):
    from vio_amd import batch_stream, stream as vs
    handle = make_handle()
    first = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=seeds[0]), nonkey_every=nonkey_every, state=(handle, 3))
    sh = first.ctx.get_stream()
    drivers = [first] + [vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=s), ctx_kwargs=dict(stream=sh), nonkey_every=nonkey_every,
                                         state=(handle, 3 + 100 * k)) for k, s in enumerate(seeds[1:], 1)]
    trajs = batch_stream.run_batched(drivers, vio.load_marg().create(stream=sh))
    return drivers, trajs


def test_stream_driver_on_a_state_slot(vio, hip_lib, est_lib):
    """Three synthetic streams through run_batched with their windows in the library's slots and in the numpy restatement behind the
    same state= interface: both slides occur (every fourth frame is no keyframe), no verdict is a failure, the trajectories agree
    within 1e-3 m (tests/test_real_imu.py's stream-level bound; the measured maximum is printed and recorded in DESIGN.md section 30)
    and lie as close to the ground truth as the drivers' own bookkeeping does."""
    from vio_amd import stream as vs
    dl, tl = run_streams(vio, hip_lib, est_lib.create)
    dr, tr = run_streams(vio, hip_lib, lambda: er.EstimatorReference(preintegrate=vio.synth.preintegrate))
    worst = 0.0
    for a, b, d in zip(tl, tr, dl):
        assert a.shape == b.shape == (6, 8)
        worst = max(worst, np.abs(a[:, 1:4] - b[:, 1:4]).max())
        assert len(d.failures) == 6 and not any(f["failure"] for f in d.failures)
        assert set(d.flags) == {vio.MARG_OLD, vio.MARG_SECOND_NEW}
    print("StreamDriver(state=): library against restatement, largest position difference %.3e m" % worst)
    assert worst <= 1e-3
    old = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=0), nonkey_every=4)
    t_old = old.run()
    assert np.abs(tl[0][:, 1:4] - t_old[:, 1:4]).max() <= 1e-3           # ... and with the host bookkeeping's closed-form prediction
    assert abs(vs.ate_rmse(tl[0], dl[0].ground_truth()) - vs.ate_rmse(t_old, old.ground_truth())) <= 1e-3


def test_stream_driver_without_state_is_untouched(vio, hip_lib):
    """Without state= the driver takes the lines it took before: state=None and no argument give the same trajectory bit for bit, no
    estimator-state library is touched, and state= with initialize= or bias_relinearize= is refused before anything is created."""
    from vio_amd import stream as vs
    a = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=5), nonkey_every=3)
    b = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=5), nonkey_every=3, state=None)
    assert a.est is None and b.est is None and np.array_equal(a.run(), b.run()) and a.failures == []
    for kw in (dict(initialize=dict(scale=1.0)), dict(bias_relinearize=(0.1, 0.01))):
        with pytest.raises(ValueError):
            vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=5), state=(object(), 0), **kw)
