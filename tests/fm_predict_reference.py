"""numpy restatement of vio_fm_predict_batch (include/vio_fm_predict.h, csrc/vio_fm_predict_math.h): VINS-Fusion's
Estimator::predictPtsInNextFrame over a track list as arrays (ids, start, depth, flag, off, pts: FmHandle.tracks_set's layout), in the
order the header writes down.  Every product and sum is one numpy operation on float64, so the device and the host build agree with it
in every bit."""
import numpy as np

D = np.float64
WINDOW = 10


def quat_to_R(q):
    """fmp_quat_to_R: q = (x, y, z, w); a (3, 3) float64."""
    x, y, z, w = (D(v) for v in q)
    tx, ty, tz = D(2) * x, D(2) * y, D(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[D(1) - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, D(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, D(1) - (txx + tyy)]], dtype=D)


def dot3(a0, a1, a2, b0, b1, b2):
    """fmp_dot: (a0 b0 + a1 b1) + a2 b2, elementwise."""
    p0, p1, p2 = a0 * b0, a1 * b1, a2 * b2
    return (p0 + p1) + p2


def mv(A, v):
    return [dot3(A[i][0], A[i][1], A[i][2], v[0], v[1], v[2]) for i in range(3)]


def tmv(A, v):
    return [dot3(A[0][i], A[1][i], A[2][i], v[0], v[1], v[2]) for i in range(3)]


def next_pose(Rp, Pp, Rc, Pc):
    """fmp_next_pose: T_next = T_cur (T_prev^-1 T_cur)."""
    Rrel = np.array([[dot3(Rp[0][i], Rp[1][i], Rp[2][i], Rc[0][j], Rc[1][j], Rc[2][j]) for j in range(3)] for i in range(3)], dtype=D)
    d = [Pc[k] - Pp[k] for k in range(3)]
    trel = tmv(Rp, d)
    Rn = np.array([[dot3(Rc[i][0], Rc[i][1], Rc[i][2], Rrel[0][j], Rrel[1][j], Rrel[2][j]) for j in range(3)] for i in range(3)], dtype=D)
    t = mv(Rc, trel)
    Pn = np.array([t[k] + Pc[k] for k in range(3)], dtype=D)
    return Rn, Pn


def qualifies(start, n_obs, depth, frame_count):
    start, n_obs, depth = np.asarray(start), np.asarray(n_obs), np.asarray(depth, dtype=D)
    return (depth > 0) & (n_obs >= 2) & (start >= 0) & (start + n_obs - 1 == frame_count)


def predict(tracks, frame_count, poses, ext, next_pose_=None):
    """tracks: dict(ids, start, depth, flag, off, pts).  Returns (ids (m,) int64, pts_cam (m, 3) float64, R_next, P_next)."""
    poses, ext = np.asarray(poses, dtype=D).reshape(11, 7), np.asarray(ext, dtype=D).reshape(7)
    ids, start, depth = np.asarray(tracks["ids"], dtype=np.int64), np.asarray(tracks["start"], dtype=np.int64), np.asarray(tracks["depth"], dtype=D)
    off, pts = np.asarray(tracks["off"], dtype=np.int64), np.asarray(tracks["pts"], dtype=D).reshape(-1, 2)
    Rn, Pn = np.zeros((3, 3)), np.zeros(3)
    if frame_count < 2 or len(ids) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3)), Rn, Pn
    R = [quat_to_R(poses[k, 3:7]) for k in range(11)]
    ric, tic = quat_to_R(ext[3:7]), ext[0:3]
    if next_pose_ is not None:
        nx = np.asarray(next_pose_, dtype=D).reshape(7)
        Rn, Pn = quat_to_R(nx[3:7]), nx[0:3].copy()
    else:
        Rn, Pn = next_pose(R[frame_count - 1], poses[frame_count - 1, 0:3], R[frame_count], poses[frame_count, 0:3])
    n_obs = off[1:] - off[:-1]
    k = np.nonzero(qualifies(start, n_obs, depth, frame_count))[0]
    out = np.zeros((len(k), 3), dtype=D)
    with np.errstate(all="ignore"):
        for s in np.unique(start[k]):                       # the rows of one start frame at once: elementwise over them
            m = np.nonzero(start[k] == s)[0]
            r = k[m]
            x, y, d = pts[off[r], 0], pts[off[r], 1], depth[r]
            pc = [d * x, d * y, d]
            pi = [a + tic[i] for i, a in enumerate(mv(ric, pc))]
            pw = [a + poses[s, i] for i, a in enumerate(mv(R[s], pi))]
            dl = [pw[i] - Pn[i] for i in range(3)]
            pl = tmv(Rn, dl)
            e = [pl[i] - tic[i] for i in range(3)]
            out[m] = np.stack(tmv(ric, e), axis=1)
    return ids[k].copy(), out, Rn, Pn
