"""Scenes of the resident Estimator state (include/vio_est.h, include/vio_est_init.h) that the CPU and the GPU tests share: states
written down directly, full batches of them, slides at the edges of k_est_slide's chunks, update cases around double2vector's
branches, and a stream's scripted life from reset to its thirtieth slide.  Plain numpy over tests/est_reference.py; nothing here
touches a GPU.  tests/test_est_scenes_cpu.py checks that every scene is what its name says."""
import math

import numpy as np

import est_init_reference as eir
import est_reference as er

NOISE = dict(acc_n=0.08, gyr_n=0.004, acc_w=4.0e-5, gyr_w=2.0e-6)
TIC, RIC_Q, G = (0.02, -0.06, 0.01), (0.5, -0.5, 0.5, 0.5), (0.0, 0.0, 9.81007)
UPDATE_TOL = 1e-12                      # relative to max(1, the compared array's largest magnitude)
CHUNK = 256                             # samples k_est_slide moves per step (EST_NT)


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def ypr(y, p, r):
    return rot([0, 0, 1], y) @ rot([0, 1, 0], p) @ rot([1, 0, 0], r)


def samples(rng, n):
    return rng.uniform(0.004, 0.006, n), rng.normal(0.0, 2.0, (n, 3)) + [0.0, 0.0, 9.81], rng.uniform(-1.0, 1.0, (n, 3))


def make_state(seed, counts, fc=10, missing=()):
    """A state written down directly: frame_count fc, counts[j] samples in interval j (none behind fc), every interval up to fc
    constructed but those in `missing`; non-zero biases, an Rs that is not orthonormal, Rs[2] / Rs[5] / Rs[8] turned by 179 degrees
    about x / y / z (the quaternion's three diagonal branches)."""
    rng = np.random.RandomState(seed)
    s = er.new_state(TIC, RIC_Q, G)
    s.update(frame_count=fc, first_imu=1)
    for i in range(11):
        s["Rs"][i] = (ypr(*rng.uniform(-60, 60, 3)) * (1.0 + 1e-3 * rng.uniform(-1, 1))).reshape(9)
    for i, ax in ((2, [1, 0, 0]), (5, [0, 1, 0]), (8, [0, 0, 1])):
        s["Rs"][i] = (rot(ax, 179.0) @ ypr(1.0, 2.0, 3.0)).reshape(9)
    s["Ps"], s["Vs"] = rng.uniform(-3, 3, (11, 3)), rng.uniform(-1, 1, (11, 3))
    s["Bas"], s["Bgs"] = rng.uniform(-0.2, 0.2, (11, 3)), rng.uniform(-0.02, 0.02, (11, 3))
    s["Headers"] = 100.0 + 0.05 * np.arange(11)
    counts = list(counts) + [0] * (11 - len(counts))
    assert all(c == 0 for c in counts[fc + 1:]) and all(counts[j] == 0 for j in missing)
    s["exists"] = np.array([int(j <= fc and j not in missing) for j in range(11)], dtype=np.int32)
    s["first"] = rng.normal(0.0, 2.0, (11, 6)) * s["exists"][:, None]
    s["lin_bias"] = np.concatenate([rng.uniform(-0.2, 0.2, (11, 3)), rng.uniform(-0.02, 0.02, (11, 3))], axis=1) * s["exists"][:, None]
    s["off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    s["dt"], s["acc"], s["gyr"] = samples(rng, int(s["off"][11]))
    s["acc_0"], s["gyr_0"] = rng.normal(0.0, 2.0, 3), rng.uniform(-1, 1, 3)
    s["last_R"], s["last_P"] = ypr(*rng.uniform(-60, 60, 3)).reshape(9), rng.uniform(-3, 3, 3)
    s["last_R0"], s["last_P0"] = ypr(*rng.uniform(-60, 60, 3)).reshape(9), rng.uniform(-3, 3, 3)
    return s


def valid_state(s):
    """vio_est_state_set's rules (include/vio_est.h) on a state dict."""
    off, fc = np.asarray(s["off"]), int(s["frame_count"])
    n = np.diff(off)
    ok = 0 <= fc <= 10 and s["first_imu"] in (0, 1) and s["failure_occur"] in (0, 1) and set(np.asarray(s["exists"]).tolist()) <= {0, 1}
    ok = ok and len(off) == 12 and off[0] == 0 and (n >= 0).all() and off[11] <= er.MAX_SAMPLES
    ok = ok and all(n[j] == 0 or (j <= fc and s["exists"][j]) for j in range(11))
    ok = ok and len(s["dt"]) == off[11] and np.asarray(s["acc"]).shape == (off[11], 3) and np.asarray(s["gyr"]).shape == (off[11], 3)
    return bool(ok and all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in s.values()))


# ---- full batches ------------------------------------------------------------------------------------------------------------------
def batch_states(count):
    """`count` distinct states for slots 0 .. count - 1: frame_count k % 11, 0 to 5 samples in every interval up to it, one slot in
    eleven (k % 11 == k // 11 % 11, so that every frame_count has one from 121 slots on) with an interval that does not exist, one
    in five with failure_occur set, headers of its own."""
    out = []
    for k in range(count):
        rng = np.random.RandomState(5000 + k)
        fc = k % 11
        hole = int(rng.randint(0, fc + 1)) if fc == (k // 11) % 11 else -1
        counts = [int(rng.randint(0, 6)) if j <= fc and j != hole else 0 for j in range(11)]
        s = make_state(6000 + k, counts, fc=fc, missing=() if hole < 0 else (hole,))
        s["failure_occur"] = int(k % 5 == 2)
        s["Headers"] = 1000.0 + k + 0.05 * np.arange(11)
        out.append(s)
    return out


# ---- slides at the edges of a chunk ------------------------------------------------------------------------------------------------
OLD_EDGES = [(5, 0), (1, 256), (256, 256), (257, 255), (255, 257), (1, 512), (300, 3796), (1, 4095), (4096, 0)]


def slide_cases():
    """(name, kind, dropped d, tail, counts): MARG_OLD with d samples in interval 0 and `tail` behind them in intervals 2, 5, 6 and
    10 (the others empty); MARG_SECOND_NEW on a full pool with interval 9 empty and interval 10 not, and with both empty."""
    out = []
    for d, tail in OLD_EDGES:
        a, b = tail // 4, tail // 3
        c = min(1, tail - a - b)
        out.append(("old_%d_%d" % (d, tail), er.MARG_OLD, d, tail, [d, 0, a, 0, 0, b, c, 0, 0, 0, tail - a - b - c]))
    out.append(("new_full_9_empty", er.MARG_SECOND_NEW, 0, 4096, [0, 1000, 0, 96, 0, 1500, 0, 0, 1000, 0, 500]))
    out.append(("new_full_both_empty", er.MARG_SECOND_NEW, 0, 4096, [6, 1000, 0, 90, 0, 1500, 0, 0, 1500, 0, 0]))
    return out


# ---- update ------------------------------------------------------------------------------------------------------------------------
def solved_window(rng, s, gauge, scale_q=False):
    """What a solve could return for state s: every frame moved by the gauge drift `gauge` and a shift, quaternions not unit if asked."""
    poses, sb, _ = er.vector2double(s)
    out = poses.copy()
    for i in range(11):
        R = gauge @ np.array(er.quat_to_rot(er.F(poses[i, 3:7] / np.linalg.norm(poses[i, 3:7])))).reshape(3, 3)
        out[i, 0:3] = gauge @ poses[i, 0:3] + [0.3, -0.2, 0.1]
        out[i, 3:7] = np.array(er.rot_to_quat(er.F(R))[0]) * ((1.0 + 0.02 * i) if scale_q else 1.0)
    sb = sb + rng.uniform(-0.01, 0.01, sb.shape)
    ext = np.concatenate([rng.uniform(-0.1, 0.1, 3), np.array(RIC_Q) * 1.01])
    return out, sb, ext


def update_case(name):
    rng = np.random.RandomState(sum(map(ord, name)))
    s = make_state(70 + len(name), [0, 2, 2])
    for i in range(11):                                      # a window of rotations (Rs[0] decides the branch)
        s["Rs"][i] = ypr(*rng.uniform(-40, 40, 3)).reshape(9)
    s["last_P"] = s["Ps"][10].copy()                         # (no gate fires: these cases are about double2vector)
    gauge = ypr(25.0, 0.0, 0.0)
    if name == "singular_old":
        s["Rs"][0] = ypr(30.0, 89.5, 10.0).reshape(9)
        gauge = ypr(25.0, 0.0, 0.0) @ rot([0, 1, 0], -40.0)   # the solved frame 0 is well away from the pole
    if name == "singular_new":
        s["Rs"][0] = ypr(30.0, 40.0, 10.0).reshape(9)
        gauge = ypr(70.0, -89.5, 0.0) @ ypr(30.0, 40.0, 10.0).T        # the solved frame 0 is ypr(70, -89.5, 0) ypr-wise near the pole
    if name == "failure_occur":
        s["failure_occur"] = 1
    out = solved_window(rng, s, gauge, scale_q=(name == "non_unit"))
    if name == "failure_occur":                              # (the window lands on last_R0 / last_P0: keep the gates quiet there too)
        s["last_P"] = er.double2vector(s, *out, False)[0]["Ps"][10].copy()
    return s, out


UPDATE_CASES = ["yaw_only", "singular_old", "singular_new", "failure_occur", "non_unit"]


def update_cases():
    """The cases tests/test_gpu_est.py's five leave open, each a dict: name, state, steps (the solved windows of one update after the
    other, the later ones built from the restatement's state), and per step the branch (singular) and the gate it must take.
      singular_by_last_R0   failure_occur set, last_R0 half a degree from the pole, Rs[0] and the solved frame 0 at 40 degrees: the
                            only kind of case where the matrix whose pitch is tested and the matrix of the product differ
      pole_in_Rs0_only      its mirror: Rs[0] half a degree from the pole, last_R0 and the solved frame not; not singular
      yaw_wrap              origin at 179 degrees of yaw, the solved frame 0 at -179: y_diff = 358
      gate_then_reanchor    the first update fires |Bas[10]| > 2.5, so the verdict itself sets failure_occur; the second must
                            re-anchor on last_R0 / last_P0 and fire nothing"""
    def base(name):
        rng = np.random.RandomState(sum(map(ord, name)))
        s = make_state(170 + len(name), [0, 2, 2])
        for i in range(11):
            s["Rs"][i] = ypr(*rng.uniform(-40, 40, 3)).reshape(9)
        return rng, s

    def quiet(s, steps):                                    # last_P where the last step's window lands
        for _ in range(2):
            t = s
            for st in steps:
                t = er.double2vector(t, *st, True)[0]
            s["last_P"] = t["Ps"][10].copy()

    out = []
    rng, s = base("singular_by_last_R0")
    s["failure_occur"] = 1
    s["Rs"][0], s["last_R0"] = ypr(30.0, 40.0, 10.0).reshape(9), ypr(-50.0, 89.5, 20.0).reshape(9)
    steps = [solved_window(rng, s, ypr(25.0, 0.0, 0.0))]
    quiet(s, steps)
    out.append(dict(name="singular_by_last_R0", state=s, steps=steps, singular=[1], gate=[0]))

    rng, s = base("pole_in_Rs0_only")
    s["failure_occur"] = 1
    s["Rs"][0], s["last_R0"] = ypr(30.0, 89.5, 10.0).reshape(9), ypr(-50.0, 35.0, 20.0).reshape(9)
    steps = [solved_window(rng, s, ypr(25.0, 0.0, 0.0) @ rot([0, 1, 0], -40.0))]
    quiet(s, steps)
    out.append(dict(name="pole_in_Rs0_only", state=s, steps=steps, singular=[0], gate=[0]))

    rng, s = base("yaw_wrap")
    s["Rs"][0] = ypr(179.0, 10.0, 5.0).reshape(9)
    steps = [solved_window(rng, s, ypr(2.0, 0.0, 0.0))]
    quiet(s, steps)
    out.append(dict(name="yaw_wrap", state=s, steps=steps, singular=[0], gate=[0]))

    rng, s = base("gate_then_reanchor")
    first = solved_window(rng, s, ypr(25.0, 0.0, 0.0))
    first[1][10, 3:6] = [3.0, 0.0, 0.0]
    t1 = er.double2vector(s, *first, True)[0]
    second = solved_window(rng, t1, ypr(-15.0, 0.0, 0.0))
    second[1][10, 3:6] = [0.01, -0.02, 0.03]
    steps = [first, second]
    quiet(s, steps)
    out.append(dict(name="gate_then_reanchor", state=s, steps=steps, singular=[0, 0], gate=[er.GATE_BA, 0]))
    return out


def branch_margin(s, poses):
    """How far the two pitch values of double2vector's branch test lie from its threshold: min | | |pitch| - 90 | - 1 |."""
    o = er.R2ypr(er.F(s["last_R0"] if s["failure_occur"] else s["Rs"][0]))
    o0 = er.R2ypr(er.quat_to_rot(er.F(poses[0, 3:7])))
    return min(abs(abs(abs(p) - 90) - 1.0) for p in (o[1], o0[1]))


# ---- a stream's life -----------------------------------------------------------------------------------------------------------------
RUNS = (0, 1, 5, 63, 64, 65, 130)
LIFE_G = (0.001, -0.002, 0.003)         # a small gravity and quiet samples: the window stays where failureDetection's gates are quiet
LIFE_RELIN = (0.0015, 0.00015)
LIFE_ROUNDS, LIFE_GATE_ROUND = 30, 7
LIFE_SLOTS = (0, 1, 63, 64, 65, 128, 254, 255)
LIFE_HEAVY = (63, 254)


def life_samples(rng, n):
    return rng.uniform(0.004, 0.006, n), rng.normal(0.0, 0.05, (n, 3)), rng.uniform(-0.3, 0.3, (n, 3))


def life_init(rng):
    """The rows of a visualInitialAlign that life() hands over: a short walk near the origin, rotations within 20 degrees, quaternions
    of norm 1.0003, a g that init_apply's product turns into LIFE_G."""
    poses, sb = np.zeros((11, 7)), np.zeros((11, 9))
    bg = rng.uniform(-0.002, 0.002, 3)
    p = rng.uniform(-0.2, 0.2, 3)
    for i in range(11):
        p = p + rng.uniform(-0.03, 0.03, 3)
        q = er.rot_to_quat(er.F(ypr(*rng.uniform(-20, 20, 3))))[0]
        poses[i] = np.concatenate([p, np.array(q) * 1.0003])
        sb[i] = np.concatenate([rng.uniform(-0.1, 0.1, 3), np.zeros(3), bg])
    R = rot(rng.uniform(-1, 1, 3), rng.uniform(20, 160))
    return poses, sb, R.T @ np.array(LIFE_G), R


def life(seed, slot_kind="normal"):
    """One stream's scripted life as a list of (call, args), as the drivers would issue them: reset; IMU runs at frame_count 0; ten
    frames of IMU runs (two of lengths from RUNS, the first window with at least one sample per interval; "heavy": one of 372 to 400
    samples) and an image call that advances, two of them behind an image call that does not; then LIFE_ROUNDS rounds on a full
    window: IMU runs, image, (the first round: init_apply with commit_last; every fourth: relinearize,) window, update, slide of
    either kind.  Round LIFE_GATE_ROUND's solved window carries |Bas[10]| = 3: the update fires a gate, a reset follows and the
    window fills again, this time with intervals that may never be constructed.
      args: imu (dt, acc, gyr); image (header, advance); update (yaw degrees, shift (3,), jitter of the speed-biases (11, 9), ext (7,),
      commit_last, fire); slide (kind, nonlinear); relinearize (ba_thresh, bg_thresh); init_apply (poses, speed_bias, g, rot, commit_last)."""
    rng = np.random.RandomState(seed)
    heavy = slot_kind == "heavy"
    script, clock = [("reset", ())], [100.0 + seed]

    def runs(must):
        lens = [int(rng.randint(372, 401))] if heavy else [RUNS[rng.randint(len(RUNS))] for _ in range(2)]
        if must and not any(lens):
            lens[-1] = 5
        for n in lens:
            script.append(("imu", life_samples(rng, n)))

    def image(advance):
        clock[0] += 0.05
        script.append(("image", (clock[0], advance)))

    def fill(must):
        stalls = set(rng.choice(np.arange(1, 10), 2, replace=False).tolist())
        for k in range(10):
            runs(must)
            if k in stalls:
                image(False)
                if not heavy:
                    runs(False)
            image(True)

    fill(True)
    first = True
    for i in range(LIFE_ROUNDS):
        runs(first)
        image(True)
        if first:
            script.append(("init_apply", life_init(rng) + (True,)))
        if i % 4 == 2:
            script.append(("relinearize", LIFE_RELIN))
        script.append(("window", ()))
        fire = i == LIFE_GATE_ROUND
        ext = np.concatenate([np.array(TIC) + rng.uniform(-0.01, 0.01, 3), np.array(RIC_Q) * (1.0 + 0.01 * rng.uniform(-1, 1))])
        script.append(("update", (float(rng.uniform(-170, 170)), rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.001, 0.001, (11, 9)), ext, True, fire)))
        first = False
        if fire:
            script.append(("reset", ()))
            fill(False)
            continue
        kind = er.MARG_SECOND_NEW if rng.uniform() < 0.3 else er.MARG_OLD
        script.append(("slide", (kind, bool(rng.randint(2)))))
    return script


def life_solved(win, args):
    """The solved window of an update call of life(): the window call's own output, every frame moved by a yaw gauge and a shift (as
    solved_window does), the speed-biases by a small jitter; `fire` sets Bas[10] = (3, 0, 0)."""
    yaw, shift, jitter, ext, _, fire = args
    gauge = ypr(yaw, 0.0, 0.0)
    poses = np.array(win["poses"], dtype=np.float64)
    out = poses.copy()
    for i in range(11):
        R = gauge @ np.array(er.quat_to_rot(er.F(poses[i, 3:7] / np.linalg.norm(poses[i, 3:7])))).reshape(3, 3)
        out[i, 0:3] = gauge @ poses[i, 0:3] + shift
        out[i, 3:7] = np.array(er.rot_to_quat(er.F(R))[0]) * (1.0 + 0.001 * i)
    sb = np.array(win["speed_bias"], dtype=np.float64) + jitter
    if fire:
        sb[10, 3:6] = [3.0, 0.0, 0.0]
    return out, sb, np.array(ext, dtype=np.float64)


def issue(handle, kind, entries, wins):
    """One call of `kind` for entries [(slot, args)] on an EstHandle or an EstimatorInitReference: one batched call, but reset, which
    the header has per slot.  wins: {slot: the last window call's result}; window writes it and update reads it.  Returns one result
    per entry (None for reset)."""
    if kind == "reset":
        for slot, _ in entries:
            handle.reset(slot)
        return [None] * len(entries)
    if kind == "imu":
        return handle.imu_batch([(slot,) + tuple(a) for slot, a in entries])
    if kind == "image":
        return handle.image_batch([(slot, a[0], a[1]) for slot, a in entries])
    if kind == "window":
        res = handle.window_batch([slot for slot, _ in entries])
        for (slot, _), r in zip(entries, res):
            wins[slot] = r
        return res
    if kind == "update":
        return handle.update_batch([(slot,) + life_solved(wins[slot], a) + (a[4],) for slot, a in entries])
    if kind == "slide":
        return handle.slide_batch([(slot, a[0], a[1]) for slot, a in entries])
    if kind == "relinearize":
        return handle.relinearize_batch([(slot, a[0], a[1]) for slot, a in entries])
    if kind == "init_apply":
        return handle.init_apply_batch([(slot,) + tuple(a) for slot, a in entries])
    raise ValueError(kind)


def life_reference():
    """The restatement behind EstHandle's methods, under life()'s config."""
    ref = eir.EstimatorInitReference()
    ref.set_config(TIC, RIC_Q, LIFE_G, NOISE)
    return ref
