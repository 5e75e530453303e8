"""A restatement of the reference's Estimator state functions (vins-mono/src/estimator.cpp) in Python floats, operation for operation
in the order include/vio_est.h writes down: clearState + setParameter (:46-103), processIMU (:105-139), the state part of processImage
(:154, :206-207), vector2double (:505-547), double2vector (:549-619), failureDetection (:645-691) and slideWindow (:1144-1264).  It is
the pin of libvio_est_hip: the reference's Estimator is not compiled by oracle/Makefile, so the library is formally unpinned and
restated from estimator.cpp.  Python's float is an IEEE double and never contracts a product into a sum, so
every function here but the ones through atan2 / sin / cos gives the bits the device gives.

A state is a dict: frame_count, first_imu, failure_occur, exists (11,), Ps (11, 3), Rs (11, 9) row-major, Vs, Bas, Bgs, Headers (11,),
tic, ric (9,), g, acc_0, gyr_0, first (11, 6), lin_bias (11, 6), last_R (9,), last_P, last_R0, last_P0, and the samples off (12,),
dt (S,), acc (S, 3), gyr (S, 3).  EstimatorReference has EstHandle's batched methods over such states, so est.BatchEstimatorState and
StreamDriver(state=) run over either.
"""
import math

import numpy as np

WINDOW_SIZE, FRAMES, MAX_SLOTS, MAX_SAMPLES = 10, 11, 256, 4096
STATUS_OK, STATUS_POOL_FULL = 0, 1
MARG_OLD, MARG_SECOND_NEW = 0, 1
GATE_NONE, GATE_BA, GATE_BG, GATE_TRANSLATION, GATE_Z = 0, 1, 2, 3, 4
DEFAULT_G = (0.0, 0.0, 9.81)
DEFAULT_NOISE = (0.2687, 0.2121, 7.07e-6, 7.07e-7)


def F(v):
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def mul33(a, b):
    """(a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j"""
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def apply33(R, v):
    return [(R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2] for i in range(3)]


def transpose33(a):
    return [a[3 * j + i] for i in range(3) for j in range(3)]


def quat_to_rot(q):
    """Eigen's toRotationMatrix on (x, y, z, w), not normalised."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def rot_to_quat(m):
    """Eigen's Quaterniond(Matrix3d): (q (x, y, z, w), branch) with branch 0 for the trace, 1 + i for diagonal i."""
    q = [0.0] * 4
    t = (m[0] + m[4]) + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
        return q, 0
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[3 * k + j] - m[3 * j + k]) * t
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q, 1 + i


def imu_step(Rs, Ps, Vs, Ba, Bg, g, acc0, gyr0, dt, acc, gyr):
    """estimator.cpp:128-135; returns the new (Rs, Ps, Vs)."""
    x0 = [acc0[c] - Ba[c] for c in range(3)]
    r = apply33(Rs, x0)
    un_acc_0 = [r[c] - g[c] for c in range(3)]
    q = [((0.5 * (gyr0[c] + gyr[c]) - Bg[c]) * dt) / 2.0 for c in range(3)] + [1.0]
    Rs = mul33(Rs, quat_to_rot(q))
    x1 = [acc[c] - Ba[c] for c in range(3)]
    r = apply33(Rs, x1)
    un_acc_1 = [r[c] - g[c] for c in range(3)]
    hdd = (0.5 * dt) * dt
    un_acc = [0.5 * (un_acc_0[c] + un_acc_1[c]) for c in range(3)]
    Ps = [Ps[c] + (dt * Vs[c] + hdd * un_acc[c]) for c in range(3)]
    Vs = [Vs[c] + dt * un_acc[c] for c in range(3)]
    return Rs, Ps, Vs


def R2ypr(R):
    n0, n1, n2, o0, o1, a0, a1 = R[0], R[3], R[6], R[1], R[4], R[2], R[5]
    y = math.atan2(n1, n0)
    cy, sy = math.cos(y), math.sin(y)
    p = math.atan2(-n2, n0 * cy + n1 * sy)
    r = math.atan2(a0 * sy - a1 * cy, -o0 * sy + o1 * cy)
    return [y / math.pi * 180.0, p / math.pi * 180.0, r / math.pi * 180.0]


def yaw_rot(y_deg):
    y = y_deg / 180.0 * math.pi
    c, s = math.cos(y), math.sin(y)
    return [c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0]


def rot_diff(R_origin, Rs0, q0):
    """(rot_diff, singular) of estimator.cpp:551-577."""
    o = R2ypr(R_origin)
    R00 = quat_to_rot(q0)
    o0 = R2ypr(R00)
    if abs(abs(o[1]) - 90) < 1.0 or abs(abs(o0[1]) - 90) < 1.0:
        return mul33(Rs0, transpose33(R00)), 1
    return yaw_rot(o[0] - o0[0]), 0


def update_frame(rd, origin_P0, pose, p0, sb):
    x, y, z, w = pose[3:7]
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    M = quat_to_rot([x / n, y / n, z / n, w / n])
    Rs = mul33(rd, M)
    r = apply33(rd, [pose[c] - p0[c] for c in range(3)])
    Ps = [r[c] + origin_P0[c] for c in range(3)]
    Vs = apply33(rd, sb[0:3])
    return Rs, Ps, Vs, list(sb[3:6]), list(sb[6:9])


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def gate(Ba10, Bg10, P10, last_P):
    if norm3(Ba10) > 2.5:
        return GATE_BA
    if norm3(Bg10) > 1.0:
        return GATE_BG
    if norm3([P10[c] - last_P[c] for c in range(3)]) > 5:
        return GATE_TRANSLATION
    if abs(P10[2] - last_P[2]) > 1:
        return GATE_Z
    return GATE_NONE


def slide_mats(back_R0, back_P0, Rs0, Ps0, ric, tic):
    r0, r1 = apply33(back_R0, tic), apply33(Rs0, tic)
    return (mul33(back_R0, ric), [back_P0[c] + r0[c] for c in range(3)], mul33(Rs0, ric), [Ps0[c] + r1[c] for c in range(3)])


# ---- states -------------------------------------------------------------------------------------------------------------------
def new_state(tic=(0, 0, 0), ric=(0, 0, 0, 1), g=DEFAULT_G):
    """A slot as vio_est_create leaves it."""
    s = dict(frame_count=0, first_imu=0, failure_occur=0, exists=np.zeros(11, dtype=np.int32), Headers=np.zeros(11), acc_0=np.zeros(3),
             gyr_0=np.zeros(3), last_R=np.zeros(9), last_P=np.zeros(3), last_R0=np.zeros(9), last_P0=np.zeros(3))
    return reset_state(s, tic, ric, g)


def reset_state(s, tic=(0, 0, 0), ric=(0, 0, 0, 1), g=DEFAULT_G):
    """clearState + setParameter (:46-103): Headers, acc_0 / gyr_0 and last_* stay."""
    s = dict(s)
    s.update(frame_count=0, first_imu=0, failure_occur=0, exists=np.zeros(11, dtype=np.int32), Ps=np.zeros((11, 3)), Vs=np.zeros((11, 3)),
             Bas=np.zeros((11, 3)), Bgs=np.zeros((11, 3)), Rs=np.tile(np.eye(3).reshape(9), (11, 1)), first=np.zeros((11, 6)),
             lin_bias=np.zeros((11, 6)), tic=np.array(F(tic)), ric=np.array(quat_to_rot(F(ric))), g=np.array(F(g)),
             off=np.zeros(12, dtype=np.int64), dt=np.zeros(0), acc=np.zeros((0, 3)), gyr=np.zeros((0, 3)))
    return s


def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def process_imu(s, dt, acc, gyr):
    """processIMU over a run; returns (new state, status)."""
    dt, acc, gyr = np.asarray(dt, dtype=np.float64).reshape(-1), np.asarray(acc, dtype=np.float64).reshape(-1, 3), np.asarray(gyr, dtype=np.float64).reshape(-1, 3)
    n, fc = len(dt), s["frame_count"]
    if fc != 0 and int(s["off"][11]) + n > MAX_SAMPLES:
        return s, STATUS_POOL_FULL
    if n == 0:
        return s, STATUS_OK
    s = copy_state(s)
    acc0, gyr0 = F(s["acc_0"]), F(s["gyr_0"])
    if not s["first_imu"]:
        s["first_imu"] = 1
        acc0, gyr0 = F(acc[0]), F(gyr[0])
    if not s["exists"][fc]:
        s["exists"][fc] = 1
        s["first"][fc] = acc0 + gyr0
        s["lin_bias"][fc] = F(s["Bas"][fc]) + F(s["Bgs"][fc])
    if fc != 0:
        Rs, Ps, Vs, Ba, Bg, g = F(s["Rs"][fc]), F(s["Ps"][fc]), F(s["Vs"][fc]), F(s["Bas"][fc]), F(s["Bgs"][fc]), F(s["g"])
        for k in range(n):
            a, w = F(acc[k]), F(gyr[k])
            Rs, Ps, Vs = imu_step(Rs, Ps, Vs, Ba, Bg, g, acc0, gyr0, float(dt[k]), a, w)
            acc0, gyr0 = a, w
        s["Rs"][fc], s["Ps"][fc], s["Vs"][fc] = Rs, Ps, Vs
        s["dt"], s["acc"], s["gyr"] = np.concatenate([s["dt"], dt]), np.concatenate([s["acc"], acc]), np.concatenate([s["gyr"], gyr])
        s["off"][fc + 1:] += n
    else:
        acc0, gyr0 = F(acc[-1]), F(gyr[-1])
    s["acc_0"], s["gyr_0"] = np.array(acc0), np.array(gyr0)
    return s, STATUS_OK


def process_image(s, header, advance):
    s = copy_state(s)
    s["Headers"][s["frame_count"]] = header
    if advance and s["frame_count"] < WINDOW_SIZE:
        s["frame_count"] += 1
    return s


def vector2double(s):
    poses, sb, ext = np.zeros((11, 7)), np.zeros((11, 9)), np.zeros(7)
    for i in range(FRAMES):
        poses[i, 0:3] = s["Ps"][i]
        poses[i, 3:7] = rot_to_quat(F(s["Rs"][i]))[0]
        sb[i, 0:3], sb[i, 3:6], sb[i, 6:9] = s["Vs"][i], s["Bas"][i], s["Bgs"][i]
    ext[0:3] = s["tic"]
    ext[3:7] = rot_to_quat(F(s["ric"]))[0]
    return poses, sb, ext


def interval_samples(s, j):
    a, b = int(s["off"][j]), int(s["off"][j + 1])
    return dict(acc0=s["first"][j, 0:3].copy(), gyr0=s["first"][j, 3:6].copy(), dt=s["dt"][a:b], acc=s["acc"][a:b], gyr=s["gyr"][a:b])


def double2vector(s, poses, sb, ext, commit_last):
    """double2vector, failureDetection and the commit of :234-237; returns (new state, failure, gate, singular)."""
    s = copy_state(s)
    poses, sb, ext = np.asarray(poses, dtype=np.float64), np.asarray(sb, dtype=np.float64), F(ext)
    Rs0 = F(s["Rs"][0])
    Ro, P0 = (F(s["last_R0"]), F(s["last_P0"])) if s["failure_occur"] else (Rs0, F(s["Ps"][0]))
    rd, singular = rot_diff(Ro, Rs0, F(poses[0, 3:7]))
    p0 = F(poses[0, 0:3])
    for i in range(FRAMES):
        s["Rs"][i], s["Ps"][i], s["Vs"][i], s["Bas"][i], s["Bgs"][i] = update_frame(rd, P0, F(poses[i]), p0, F(sb[i]))
    s["tic"], s["ric"] = np.array(ext[0:3]), np.array(quat_to_rot(ext[3:7]))
    gt = gate(F(s["Bas"][10]), F(s["Bgs"][10]), F(s["Ps"][10]), F(s["last_P"]))
    s["failure_occur"] = int(gt != 0)
    if gt == 0 and commit_last:
        s["last_R"], s["last_P"], s["last_R0"], s["last_P0"] = s["Rs"][10].copy(), s["Ps"][10].copy(), s["Rs"][0].copy(), s["Ps"][0].copy()
    return s, int(gt != 0), gt, singular


def slide_window(s, kind):
    """slideWindow; returns (new state, slid, (marg_R, marg_P, new_R, new_P) or None)."""
    if s["frame_count"] != WINDOW_SIZE:
        return s, 0, None
    s = copy_state(s)
    if kind == MARG_OLD:
        back_R0, back_P0 = F(s["Rs"][0]), F(s["Ps"][0])
        for k in ("Rs", "Ps", "Vs", "Bas", "Bgs", "Headers", "exists", "first", "lin_bias"):
            s[k][0:10] = s[k][1:11].copy()          # (frame 10 stays: it is the copy of the new frame 9)
        d = int(s["off"][1])
        s["dt"], s["acc"], s["gyr"] = s["dt"][d:], s["acc"][d:], s["gyr"][d:]
        s["off"] = np.concatenate([s["off"][1:] - d, [s["off"][11] - d]])
        mats = slide_mats(back_R0, back_P0, F(s["Rs"][0]), F(s["Ps"][0]), F(s["ric"]), F(s["tic"]))
    else:
        s["off"][10] = s["off"][11]
        for k in ("Rs", "Ps", "Vs", "Bas", "Bgs", "Headers"):
            s[k][9] = s[k][10]
        mats = None
    s["exists"][10] = 1
    s["first"][10] = np.concatenate([s["acc_0"], s["gyr_0"]])
    s["lin_bias"][10] = np.concatenate([s["Bas"][10], s["Bgs"][10]])
    return s, 1, mats


class EstimatorReference:
    """EstHandle's methods over the restatement: what est.BatchEstimatorState and StreamDriver(state=) need of a handle."""

    def __init__(self, preintegrate=None):
        """preintegrate: synth.preintegrate, for window_batch's records (None: window_batch gives no records)."""
        self.preintegrate = preintegrate
        self.cfg = dict(tic=(0, 0, 0), ric=(0, 0, 0, 1), g=DEFAULT_G)
        self.noise = dict(zip(("acc_n", "gyr_n", "acc_w", "gyr_w"), DEFAULT_NOISE))
        self.state = {}

    def _s(self, slot):
        if slot not in self.state:
            self.state[slot] = new_state(**self.cfg)
        return self.state[slot]

    def set_config(self, tic=(0, 0, 0), ric=(0, 0, 0, 1), g=DEFAULT_G, noise=DEFAULT_NOISE):
        self.cfg = dict(tic=tic, ric=ric, g=g)
        self.noise = dict(noise) if isinstance(noise, dict) else dict(zip(("acc_n", "gyr_n", "acc_w", "gyr_w"), noise))

    def reset(self, slot):
        self.state[slot] = reset_state(self._s(slot), **self.cfg)

    def state_set(self, slot, state):
        s = copy_state(state)
        s["exists"] = np.asarray(s["exists"], dtype=np.int32)[:11].copy()
        for k, v in dict(off=np.zeros(12, dtype=np.int64), dt=np.zeros(0), acc=np.zeros((0, 3)), gyr=np.zeros((0, 3))).items():
            s.setdefault(k, v)
        self.state[slot] = s

    def state_get(self, slot):
        return copy_state(self._s(slot))

    @staticmethod
    def _res(s, **kw):
        r = dict(status=0, frame_count=s["frame_count"], n_samples=0, failure=0, gate=0, singular=0, slid=0, shift_depth=0,
                 marg_R=np.zeros((3, 3)), marg_P=np.zeros(3), new_R=np.zeros((3, 3)), new_P=np.zeros(3))
        r.update(kw)
        return r

    def imu_batch(self, items):
        out = []
        for slot, dt, acc, gyr in items:
            s, st = process_imu(self._s(slot), dt, acc, gyr)
            self.state[slot] = s
            out.append(self._res(s, status=st, n_samples=int(s["off"][11])))
        return out

    def image_batch(self, items):
        out = []
        for slot, header, advance in items:
            self.state[slot] = process_image(self._s(slot), header, advance)
            out.append(self._res(self.state[slot]))
        return out

    def window_batch(self, slots):
        out = []
        for slot in slots:
            s = self._s(slot)
            poses, sb, ext = vector2double(s)
            pre = []
            for j in range(1, FRAMES if self.preintegrate else 1):
                iv = interval_samples(s, j)
                lb = s["lin_bias"][j] if s["exists"][j] else np.zeros(6)
                pre.append(self.preintegrate(iv["acc0"], iv["gyr0"], lb[0:3].copy(), lb[3:6].copy(), list(iv["dt"]), list(iv["acc"]),
                                             list(iv["gyr"]), **self.noise))
            out.append(self._res(s, poses=poses, speed_bias=sb, ext=ext, preint=pre))
        return out

    def update_batch(self, items):
        out = []
        for slot, poses, sb, ext, commit in items:
            s, failure, gt, singular = double2vector(self._s(slot), poses, sb, ext, commit)
            self.state[slot] = s
            p2, sb2, ext2 = vector2double(s)
            out.append(self._res(s, failure=failure, gate=gt, singular=singular, poses=p2, speed_bias=sb2, ext=ext2))
        return out

    def slide_batch(self, items):
        out = []
        for slot, kind, nonlinear in items:
            s, slid, mats = slide_window(self._s(slot), kind)
            self.state[slot] = s
            r = self._res(s, slid=slid, n_samples=int(s["off"][11]))
            if mats is not None:
                r.update(marg_R=np.array(mats[0]).reshape(3, 3), marg_P=np.array(mats[1]), new_R=np.array(mats[2]).reshape(3, 3),
                         new_P=np.array(mats[3]), shift_depth=int(bool(nonlinear)))
            out.append(r)
        return out
