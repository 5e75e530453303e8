"""include/vio_est_init.h on the GPU (libvio_est_hip.so: k_est_init_apply, k_est_relinearize) against tests/est_init_reference.py through
state_get, bit for bit: visualInitialAlign's hand-over into full slots of 0 to 4096 samples, the device rule (a window that is not
full, a missing interval) beside served slots, independence of batch and slot index, the records of the next window call against
libvio_imu_hip byte for byte (one kernel text), the re-linearisation at, one ulp above and below its thresholds, the argument rules,
and the stream drivers that live in a slot from their first sample.  A missing library is a failure, not a skip."""
import ctypes as C

import numpy as np
import pytest

import est_init_reference as eir
import est_reference as er
from test_est_init_cpu import RELIN, biased
from test_est_init_reference import RELIN_CASES, T_A, T_G, init_inputs
from test_gpu_est import NOISE, differing, eh, est_lib, imu_records, make_state, samples, seed_slots, vec, window_intervals  # noqa: F401  (two are fixtures)

pytestmark = pytest.mark.gpu

SLOTS = (0, 7, 255)
TOTALS = {0: [0] * 11, 1: [0] * 10 + [1], 63: [0, 3, 20, 1, 0, 7, 0, 2, 9, 1, 20], 64: [0, 64] + [0] * 9, 65: [0, 3, 20, 1, 0, 7, 0, 2, 9, 2, 21],
          4096: [0] + [400] * 9 + [496]}
Q_NORM = 1.0003


def window_bytes(r):
    return b"".join(bytes(p) for p in r["preint"])


# ---- 1. init_apply_batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", sorted(TOTALS))
def test_init_apply_is_the_restatement_bit_for_bit_and_the_samples_stay(eh, total):
    assert sum(TOTALS[total]) == total
    states = [make_state(200 + total % 97 + k, TOTALS[total]) for k in range(3)]
    seed_slots(eh, states)
    ins = [init_inputs(10 * total % 89 + k, Q_NORM) for k in range(3)]
    for poses, sb, g, R in ins:                             # a quaternion that is not unit, a proper rotation, g not along z
        assert abs(np.linalg.norm(poses[3, 3:7]) - Q_NORM) < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(g[0:2]).max() > 1e-3
    res = eh.init_apply_batch([(slot,) + i for slot, i in zip(SLOTS, ins)])
    for slot, s, i, r in zip(SLOTS, states, ins, res):
        want, st = eir.init_apply(s, *i)
        assert (r["status"], r["frame_count"], st) == (0, 10, 0)
        got = eh.state_get(slot)
        assert differing(got, want) == [], (slot, total)
        assert got["off"][11] == total and np.array_equal(got["last_P"], s["last_P"])
    again = eh.init_apply_batch([(slot,) + i + (True,) for slot, i in zip(SLOTS, ins)])      # repeated, and commit_last
    for slot, s, i in zip(SLOTS, states, ins):
        assert differing(eh.state_get(slot), eir.init_apply(s, *i, commit_last=True)[0]) == [], (slot, total)
    assert [r["status"] for r in again] == [0, 0, 0]


def test_a_window_that_is_not_ready_stays_and_its_neighbours_are_served(eh):
    short = make_state(301, [0, 3, 20, 1, 0, 7, 0, 2, 9, 2], fc=9)
    hole = make_state(302, [0, 3, 20, 0, 0, 7, 0, 2, 9, 2, 21], missing=(3,))
    good = make_state(303, [0, 3, 20, 1, 0, 7, 0, 2, 9, 2, 21])
    slots, twins = (4, 5, 6, 254), (104, 105)
    seed_slots(eh, [short, good, hole, good], slots)
    seed_slots(eh, [short, hole], twins)                    # the untouched twins
    ins = [init_inputs(40 + k, Q_NORM) for k in range(4)]
    res = eh.init_apply_batch([(slot,) + i for slot, i in zip(slots, ins)])
    assert [r["status"] for r in res] == [eir.STATUS_NOT_READY, 0, eir.STATUS_NOT_READY, 0] and [r["frame_count"] for r in res] == [9, 10, 10, 10]
    for slot, twin, s in ((4, 104, short), (6, 105, hole)):
        assert differing(eh.state_get(slot), eh.state_get(twin)) == [] and differing(eh.state_get(slot), s) == [], slot
    for slot, i in ((5, ins[1]), (254, ins[3])):
        assert differing(eh.state_get(slot), eir.init_apply(good, *i)[0]) == [], slot
    assert eir.init_apply(short, *ins[0])[1] == eir.init_apply(hole, *ins[2])[1] == eir.STATUS_NOT_READY


def test_a_slots_bytes_depend_neither_on_the_batch_nor_on_the_slot(eh):
    """65 slots in one call (more than a wavefront's worth of items), two, and one: each equals the same item alone in another slot."""
    states = [make_state(400 + k, [0, 1, 2, 0, 3, 0, 1, 0, 2, 1, k % 5]) for k in range(65)]
    ins = [init_inputs(500 + k, Q_NORM) + (bool(k % 2),) for k in range(65)]
    alone = []
    for k in range(65):
        slot = 255 - 2 * k
        eh.state_set(slot, states[k])
        assert eh.init_apply_batch([(slot,) + ins[k]])[0]["status"] == 0
        g = eh.state_get(slot)
        assert differing(g, eir.init_apply(states[k], *ins[k][:4], commit_last=ins[k][4])[0]) == [], k
        alone.append(g)
    for B in (1, 2, 65):
        slots = list(range(B))
        seed_slots(eh, states[:B], slots)
        res = eh.init_apply_batch([(slot,) + ins[slot] for slot in slots])
        assert [r["status"] for r in res] == [0] * B
        for slot in slots:
            assert differing(eh.state_get(slot), alone[slot]) == [], (B, slot)


def test_the_handed_over_window_is_the_imu_librarys_at_zero_and_bg_and_runs_on(vio, eh):
    """After the hand-over the window call's records are ImuHandle.propagate's of the same samples at (0, bg), byte for byte, and
    update, slide and processIMU run on the slot as on one seeded with the restatement's state."""
    s = make_state(601, [0, 3, 20, 1, 0, 7, 0, 65, 2, 200, 21])
    s["last_P"] = np.zeros(3)
    i = init_inputs(602, Q_NORM)
    want, _ = eir.init_apply(s, *i, commit_last=True)
    seed_slots(eh, [s, want], (11, 12))
    assert eh.init_apply_batch([(11,) + i + (True,)])[0]["status"] == 0
    wins = eh.window_batch([11, 12])
    ivs, lb = window_intervals(want)
    assert np.array_equal(lb[:, 0:3], np.zeros((10, 3))) and np.array_equal(lb[:, 3:6], i[1][1:, 6:9])
    same_kernel = imu_records(vio, ivs, lb)
    assert [bytes(p) for p in wins[0]["preint"]] == same_kernel and window_bytes(wins[0]) == window_bytes(wins[1])
    assert wins[0]["poses"].tobytes() == wins[1]["poses"].tobytes() == er.vector2double(want)[0].tobytes()
    run = samples(np.random.RandomState(3), 30)
    outs = []
    for slot, w in zip((11, 12), wins):
        u = eh.update_batch([(slot, w["poses"], w["speed_bias"], w["ext"], True)])[0]
        sl = eh.slide_batch([(slot, er.MARG_OLD, True)])[0]
        im = eh.imu_batch([(slot,) + run])[0]
        assert (u["failure"], sl["slid"], im["status"]) == (0, 1, 0)
        outs.append(eh.state_get(slot))
    assert differing(outs[0], outs[1]) == [] and outs[0]["off"][11] == 319 + 30


# ---- 2. relinearize_batch -------------------------------------------------------------------------------------------------------
def relin_state(seed, placed, fc=10, missing=(), counts=(0, 3, 20, 1, 0, 7, 0, 65, 2, 30, 21)):
    """A state whose intervals' linearisation biases equal their start frames' biases (nothing would move), but for the intervals of
    `placed`: {j: index into RELIN_CASES}."""
    counts = [c if j <= fc and j not in missing else 0 for j, c in enumerate(counts)]
    s = make_state(seed, counts, fc=fc, missing=missing)
    for j, k in placed.items():
        s["Bas"][j - 1], s["Bgs"][j - 1] = RELIN_CASES[k][1], RELIN_CASES[k][2]
    for j in range(1, 11):
        if s["exists"][j]:
            s["lin_bias"][j] = RELIN_CASES[placed[j]][3] if j in placed else np.concatenate([s["Bas"][j - 1], s["Bgs"][j - 1]])
    return s


def test_relinearize_at_its_thresholds(vio, eh):
    """One call over six slots, each with its own thresholds: a difference exactly at the threshold and one ulp above it for either
    bias, a negative one, only ba and only bg, a missing interval, a window that is not full, thresholds 0 with equal biases and with
    one ulp between them; intervals 1 and 10 among the moved.  Mask, count and state against the restatement; the second call reports
    nothing; the next window's records are the IMU library's at the new biases and the untouched intervals' records are unchanged."""
    ta, tg = RELIN_CASES[0][4], RELIN_CASES[2][5]
    cases = [(relin_state(701, {3: 0, 1: 1}), ta, T_G, 1 << 1),
             (relin_state(702, {4: 2, 10: 3}), T_A, tg, 1 << 10),
             (relin_state(703, {1: 4, 2: 5, 5: 6, 10: 7}, missing=(7,)), T_A, T_G, (1 << 1) | (1 << 5) | (1 << 10)),
             (relin_state(704, {}), 0.0, 0.0, 0),
             (relin_state(705, {6: 9}), 0.0, 0.0, 1 << 6),
             (relin_state(706, {}, fc=6), T_A, T_G, 0b1111110)]
    assert np.abs(cases[2][0]["Bas"][6]).max() > 0 and not cases[2][0]["lin_bias"][7].any()     # (frame 6 is away from the missing interval 7's zeros)
    cases[5][0]["Bas"][0:6] += 0.5                          # every interval of the short window has moved
    slots = (0, 1, 63, 64, 200, 255)
    seed_slots(eh, [c[0] for c in cases], slots)
    before = eh.window_batch(list(slots))
    res = eh.relinearize_batch([(slot, c[1], c[2]) for slot, c in zip(slots, cases)])
    after = []
    for slot, (s, a, g, mask), r in zip(slots, cases, res):
        want, n, m = eir.relinearize(s, a, g)
        assert m == mask and n == bin(mask).count("1"), slot
        assert (r["status"], r["frame_count"], r["n_relinearized"], r["mask"]) == (0, s["frame_count"], n, mask), slot
        assert differing(eh.state_get(slot), want) == [], slot
        after.append(want)
    assert [(r["n_relinearized"], r["mask"]) for r in eh.relinearize_batch([(slot, c[1], c[2]) for slot, c in zip(slots, cases)])] == [(0, 0)] * 6
    wins = eh.window_batch(list(slots))
    for slot, want, (_, _, _, mask), w0, w1 in zip(slots, after, cases, before, wins):
        assert differing(eh.state_get(slot), want) == [], slot
        ivs, lb = window_intervals(want)
        recs = imu_records(vio, ivs, lb)
        for j in range(1, 11):
            got = bytes(w1["preint"][j - 1])
            assert got == recs[j - 1], (slot, j)
            moved = bool(mask >> j & 1)
            assert (got != bytes(w0["preint"][j - 1])) == moved, (slot, j)
            if moved:
                assert np.array_equal(vec(w1["preint"][j - 1])[11:17], np.concatenate([want["Bas"][j - 1], want["Bgs"][j - 1]]))


# ---- 3. argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing_launch_nothing_and_name_the_item(vio, eh):
    e = vio.est
    states = [make_state(800 + k, TOTALS[65]) for k in range(3)]
    seed_slots(eh, states)
    eh.window_batch([0])
    timing = eh.timing()                                    # (of the last call that launched)
    ok = init_inputs(801, Q_NORM)
    res, rres = (e.VioEstResult * 4)(), (e.VioEstRelinResult * 4)()

    def init_items(entries):
        arr = (e.VioEstInitItem * len(entries))()
        for k, (slot, poses, sb, g, R) in enumerate(entries):
            arr[k].slot = slot
            for name, v in (("poses", poses), ("speed_bias", sb), ("g", g), ("rot", R)):
                v = np.ascontiguousarray(v, dtype=np.float64)
                C.memmove(C.addressof(getattr(arr[k], name)), v.ctypes.data, v.nbytes)
        return arr

    def relin_items(entries):
        return (e.VioEstRelinItem * len(entries))(*[e.VioEstRelinItem(slot, 0, a, g) for slot, a, g in entries])

    nan_pose, inf_rot, nan_g, nan_sb = ok[0].copy(), ok[3].copy(), ok[2].copy(), ok[1].copy()
    nan_pose[10, 6], inf_rot[2, 2], nan_g[0], nan_sb[0, 0] = np.nan, np.inf, np.nan, np.nan
    bad_init = [[(0,) + ok, (256,) + ok], [(0,) + ok, (-1,) + ok], [(0,) + ok, (7,) + ok, (0,) + ok], [(0,) + ok, (7, nan_pose) + ok[1:]],
                [(0,) + ok, (7, ok[0], nan_sb) + ok[2:]], [(0,) + ok, (7, ok[0], ok[1], nan_g, ok[3])], [(0,) + ok, (7,) + ok[:3] + (inf_rot,)]]
    for k, entries in enumerate(bad_init):
        items = init_items(entries)
        assert eh.lib.fn["init_apply_batch"](eh.h, C.c_int32(len(entries)), C.addressof(items), C.addressof(res)) == -1, k
        assert "init_apply_batch" in eh.last_error() and "item %d" % (len(entries) - 1) in eh.last_error(), (k, eh.last_error())
    bad_relin = [[(0, 0.1, 0.01), (256, 0.1, 0.01)], [(0, 0.1, 0.01), (0, 0.1, 0.01)], [(0, 0.1, 0.01), (7, -1e-300, 0.01)],
                 [(0, 0.1, 0.01), (7, 0.1, float("nan"))], [(0, 0.1, 0.01), (7, float("inf"), 0.01)], [(0, 0.1, 0.01), (7, 0.1, -0.01)]]
    for k, entries in enumerate(bad_relin):
        items = relin_items(entries)
        assert eh.lib.fn["relinearize_batch"](eh.h, C.c_int32(len(entries)), C.addressof(items), C.addressof(rres)) == -1, k
        assert "relinearize_batch" in eh.last_error() and "item 1" in eh.last_error(), (k, eh.last_error())
    one, rone = init_items([(0,) + ok]), relin_items([(0, 0.1, 0.01)])
    for name, items, out in (("init_apply_batch", one, res), ("relinearize_batch", rone, rres)):
        assert eh.lib.fn[name](eh.h, C.c_int32(1), None, C.addressof(out)) == -1 and "NULL" in eh.last_error()
        assert eh.lib.fn[name](eh.h, C.c_int32(1), C.addressof(items), None) == -1 and "NULL" in eh.last_error()
        assert eh.lib.fn[name](eh.h, C.c_int32(257), C.addressof(items), C.addressof(out)) == -1 and eh.lib.fn[name](eh.h, C.c_int32(-1), C.addressof(items), C.addressof(out)) == -1
    for call in (lambda: eh.init_apply_batch([(0,) + ok, (0,) + ok]), lambda: eh.relinearize_batch([(3, 0.1, 0.01), (300, 0.1, 0.01)])):
        with pytest.raises(vio.VioError) as exc:
            call()
        assert exc.value.status == -1
    assert eh.timing() == timing                            # nothing launched
    for slot, s in zip(SLOTS, states):
        assert differing(eh.state_get(slot), s) == [], slot
    assert eh.init_apply_batch([]) == [] and eh.relinearize_batch([]) == []


# ---- 4. the drivers ----------------------------------------------------------------------------------------------------------------
def test_three_streams_live_in_their_slots_from_the_first_sample(vio, hip_lib, est_lib):
    """Three drivers through run_batched with initialize=dict(sfm=True, all_frames=, state=) and features=, against the same three
    without `state` at tests/test_stream.py's bar between two implementations: positions within 1e-3 m and the ATE (ate_rmse, as
    there) within 1 %.  The same bar holds the three to themselves run alone (the rounding of the two marginalisation tails,
    batch_stream.py) and those to the comparator that shares the slot's rule for a new interval, bias_relinearize= at thresholds
    that never fire (run alone: run_batched does not batch that option).
    The aligned APE is printed and not asserted.  These streams' APE is 0.3 to 0.5 mm (SfM needs 0.1 px noise), and 1 % of it lies
    below what the same driver gives through run and run_batched: first device run, second stream, 3.376e-4 m batched against
    3.306e-4 m alone (2.1 %, positions apart by 2.9e-5 m), 3.414e-4 m for the comparator (positions 4.9e-5 m from the slot's), and
    5.411e-4 m without `state` (positions 6.1e-4 m: its new intervals are linearised at zero bias)."""
    from vio_amd import batch_stream, stream as vs
    make = lambda s: vs.SyntheticStream(n_frames=14, landmarks_per_frame=60, track_len=10, seed=s, pixel_noise=0.1 / 460.0)     # noqa: E731
    ah, fh, est = vio.load_aif().create(), vio.load_fm().create(), est_lib.create()
    try:
        def group(base, est_base, **kw):
            ds, sh = [], None
            for k in range(3):
                init = dict(sfm=True, all_frames=(ah, base + k))
                if est_base is not None:
                    init["state"] = (est, est_base + 100 * k)
                extra = dict(kw, ctx_kwargs=dict(stream=sh)) if sh is not None else dict(kw)
                ds.append(vs.StreamDriver(hip_lib, make(k), seed=2, triangulate=True, initialize=init, features=(fh, base + k), **extra))
                sh = ds[0].ctx.get_stream()
            return ds, sh
        dd, sh = group(10, 3)
        td = batch_stream.run_batched(dd, vio.load_marg().create(stream=sh))
        dp, sh = group(20, None)
        tp = batch_stream.run_batched(dp, vio.load_marg().create(stream=sh))
        da, _ = group(40, 4)
        ta = [d.run() for d in da]
        dn, _ = group(30, None, bias_relinearize=(1e9, 1e9))
        tn = [d.run() for d in dn]
        for d, p, a, n, x, y, w, z in zip(dd, dp, da, dn, td, tp, ta, tn):
            assert d.init_tries == p.init_tries == a.init_tries == n.init_tries and d.init_frame == p.init_frame == a.init_frame == n.init_frame
            assert len(x) == len(y) == len(w) == len(z) == 14 - d.init_frame
            for q in (d, a):
                assert len(q.failures) == len(x) and not any(f["failure"] for f in q.failures)
                s = est.state_get(q.est_slot)
                assert s["frame_count"] == 10 and np.array_equal(s["last_P"], s["Ps"][10])
            ex, ey, ew, ez = (vs.ape_stats(t, q.ground_truth())["rmse"] for t, q in ((x, d), (y, p), (w, a), (z, n)))
            ax, ay, aw, az = (vs.ate_rmse(t, q.ground_truth()) for t, q in ((x, d), (y, p), (w, a), (z, n)))
            dplain, dalone, dnever = (np.abs(u[:, 1:4] - v[:, 1:4]).max() for u, v in ((x, y), (x, w), (w, z)))
            print("slot %d: max |dP| %.3e m (batched, without state) %.3e m (batched against alone) %.3e m (alone, bias_relinearize that never fires); "
                  "aligned APE %.6e batched, %.6e without state, %.6e alone, %.6e never fires" % (d.est_slot, dplain, dalone, dnever, ex, ey, ew, ez))
            assert dplain < 1e-3 and dalone < 1e-3 and dnever < 1e-3
            assert abs(ax - ay) <= 0.01 * ay and abs(ax - aw) <= 0.01 * aw and abs(aw - az) <= 0.01 * az
    finally:
        for h in (ah, fh, est):
            h.close()


def test_the_slot_relinearises_where_the_imu_library_would(vio, hip_lib, est_lib):
    """state=dict(relinearize=) against bias_relinearize= on a stream with a constant IMU bias: the same count at every step, some
    steps with and some without, and trajectories within tests/test_stream.py's position bar."""
    from vio_amd import stream as vs
    est = est_lib.create()
    try:
        plain = vs.StreamDriver(hip_lib, biased(vio), seed=2, bias_relinearize=RELIN)
        tp = plain.run()
        drv = vs.StreamDriver(hip_lib, biased(vio), seed=2, state=dict(handle=est, slot=9, relinearize=RELIN))
        td = drv.run()
        print("repropagated: IMU library %s, slot %s" % (plain.repropagated, drv.repropagated))
        assert not hasattr(drv, "imu_h") and drv.repropagated == plain.repropagated and len(td) == len(tp) == len(drv.repropagated)
        assert any(n > 0 for n in drv.repropagated) and any(n == 0 for n in drv.repropagated)
        assert np.abs(td[:, 1:4] - tp[:, 1:4]).max() < 1e-3
    finally:
        est.close()
