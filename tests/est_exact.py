"""double2vector (vins-mono/src/estimator.cpp:549-619) in mpmath at 50 digits, written from the reference's lines and its
utility.h (R2ypr, ypr2R) and from Eigen's documented quaternion conversions, not from csrc/vio_est_math.h: a second opinion on
tests/est_reference.py, whose restatement shares a header with the kernel.  It takes the doubles the library takes (exactly, as
mpmath numbers), rounds nothing on the way and returns doubles rounded once at the end.

    out = double2vector(state, poses, speed_bias)      # dict: Rs (11, 9), Ps (11, 3), Vs (11, 3), quats (11, 4) xyzw of Rs,
                                                       #       pitch (origin, solved frame 0) in degrees, y_diff, singular
"""
import numpy as np
from mpmath import mp, mpf

DIGITS = 50


def _mat(v):
    v = np.asarray(v, dtype=np.float64).reshape(3, 3)
    return [[mpf(float(v[i, j])) for j in range(3)] for i in range(3)]


def _vec(v):
    return [mpf(float(x)) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def _mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _apply(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _T(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def R2ypr(R):
    """utility.h:66-81, degrees."""
    n, o, a = [R[i][0] for i in range(3)], [R[i][1] for i in range(3)], [R[i][2] for i in range(3)]
    y = mp.atan2(n[1], n[0])
    p = mp.atan2(-n[2], n[0] * mp.cos(y) + n[1] * mp.sin(y))
    r = mp.atan2(a[0] * mp.sin(y) - a[1] * mp.cos(y), -o[0] * mp.sin(y) + o[1] * mp.cos(y))
    return [y / mp.pi * 180, p / mp.pi * 180, r / mp.pi * 180]


def ypr2R(y, p, r):
    """utility.h:84-108: Rz Ry Rx from degrees."""
    y, p, r = y / 180 * mp.pi, p / 180 * mp.pi, r / 180 * mp.pi
    Rz = [[mp.cos(y), -mp.sin(y), 0], [mp.sin(y), mp.cos(y), 0], [0, 0, 1]]
    Ry = [[mp.cos(p), 0, mp.sin(p)], [0, 1, 0], [-mp.sin(p), 0, mp.cos(p)]]
    Rx = [[1, 0, 0], [0, mp.cos(r), -mp.sin(r)], [0, mp.sin(r), mp.cos(r)]]
    return _mul(_mul(Rz, Ry), Rx)


def to_rotation_matrix(x, y, z, w):
    """Quaterniond(w, x, y, z).toRotationMatrix(): the quaternion is not normalised."""
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def from_rotation_matrix(m):
    """Quaterniond(Matrix3d): the trace branch where the trace is positive, the largest diagonal entry otherwise; (x, y, z, w)."""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [mpf(0)] * 4
    if t > 0:
        t = mp.sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t
        return q
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = mp.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
    q[i] = t / 2
    t = 1 / (2 * t)
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q


def double2vector(state, poses, speed_bias):
    poses, sb = np.asarray(poses, dtype=np.float64).reshape(11, 7), np.asarray(speed_bias, dtype=np.float64).reshape(11, 9)
    with mp.workdps(DIGITS):
        Rs0 = _mat(state["Rs"][0])
        origin_R0, origin_P0 = R2ypr(Rs0), _vec(state["Ps"][0])                    # :551-552
        if state["failure_occur"]:                                                # :554-559
            origin_R0, origin_P0 = R2ypr(_mat(state["last_R0"])), _vec(state["last_P0"])
        x0, y0, z0, w0 = _vec(poses[0, 3:7])
        R00 = to_rotation_matrix(x0, y0, z0, w0)                                   # :560-564, not normalised
        origin_R00 = R2ypr(R00)
        y_diff = origin_R0[0] - origin_R00[0]                                      # :565
        rot_diff = ypr2R(y_diff, mpf(0), mpf(0))                                   # :567
        singular = bool(abs(abs(origin_R0[1]) - 90) < 1 or abs(abs(origin_R00[1]) - 90) < 1)
        if singular:                                                              # :568-577: Rs[0], also where failure_occur is set
            rot_diff = _mul(Rs0, _T(R00))
        p0 = _vec(poses[0, 0:3])
        Rs, Ps, Vs, qs = np.zeros((11, 9)), np.zeros((11, 3)), np.zeros((11, 3)), np.zeros((11, 4))
        for i in range(11):                                                       # :579-600
            x, y, z, w = _vec(poses[i, 3:7])
            n = mp.sqrt(x * x + y * y + z * z + w * w)
            R = _mul(rot_diff, to_rotation_matrix(x / n, y / n, z / n, w / n))
            p = _vec(poses[i, 0:3])
            P = _apply(rot_diff, [p[c] - p0[c] for c in range(3)])
            V = _apply(rot_diff, _vec(sb[i, 0:3]))
            Rs[i] = [float(R[a][b]) for a in range(3) for b in range(3)]
            Ps[i] = [float(P[c] + origin_P0[c]) for c in range(3)]
            Vs[i] = [float(v) for v in V]
            qs[i] = [float(v) for v in from_rotation_matrix(R)]
        return dict(Rs=Rs, Ps=Ps, Vs=Vs, quats=qs, pitch=(float(origin_R0[1]), float(origin_R00[1])), y_diff=float(y_diff), singular=int(singular))
