"""A plain Python / numpy restatement of the reference's FeatureManager (VM/src/feature_manager.cpp) over a list of dicts
(id, start, depth, flag, pts (k, 2)), the form tests/fm_util.py gives the golden tracks: what libvio_fm_hip (include/vio_fm.h) is held
to.  Integer and copy work is exact; the two floating-point pieces are written as csrc/vio_fm_math.h writes them (Python floats are
IEEE doubles, no contraction), and the parallax sum comes in both orders: the reference's list order and the device's fixed order.
Triangulation is a numpy SVD like the reference's (not bitwise anything: TRI_RTOL)."""
import math

import numpy as np

WINDOW_SIZE = 10
MAX_TRACKS, MAX_POINTS, MAX_OBS, NT = 2048, 1024, 11, 1024
INIT_DEPTH, MIN_PARALLAX = 5.0, 10.0 / 460.0
STATUS_OK, STATUS_TABLE_FULL, STATUS_GAP, STATUS_OBS_FULL = 0, 1, 2, 3
BACK_SHIFT_DEPTH, BACK, FRONT = 0, 1, 2


def copy_tracks(tracks):
    return [dict(id=int(t["id"]), start=int(t["start"]), depth=float(t["depth"]), flag=int(t.get("flag", 0)),
                 pts=np.array(t["pts"], dtype=np.float64).reshape(-1, 2)) for t in tracks]


def usable(t):
    return len(t["pts"]) >= 2 and t["start"] < WINDOW_SIZE - 2


def counts(tracks):
    u = [t for t in tracks if usable(t)]
    return len(tracks), len(u), sum(len(t["pts"]) - 1 for t in u)


def parallax_term(pi, pj):
    ui, vi = float(pi[0]) / 1.0, float(pi[1]) / 1.0
    du, dv = ui - float(pj[0]), vi - float(pj[1])
    return math.sqrt(du * du + dv * dv)


def parallax_terms(tracks, frame_count):
    """One term per row, None where addFeatureCheckParallax's loop skips the row (:79-80)."""
    out = []
    for t in tracks:
        k = len(t["pts"])
        if t["start"] <= frame_count - 2 and t["start"] + k - 1 >= frame_count - 1:
            out.append(parallax_term(t["pts"][frame_count - 2 - t["start"]], t["pts"][frame_count - 1 - t["start"]]))
        else:
            out.append(None)
    return out


def sum_reference_order(terms):
    s = 0.0
    for v in terms:
        if v is not None:
            s += v
    return s


def sum_device_order(terms):
    """include/vio_fm.h: thread t of 1024 sums its rows t, t + 1024 in that order from 0.0, then s[t] += s[t + w], w = 512 .. 1."""
    s = [0.0] * NT
    for r, v in enumerate(terms):
        if v is not None:
            s[r % NT] = s[r % NT] + v
    w = NT // 2
    while w >= 1:
        for t in range(w):
            s[t] = s[t] + s[t + w]
        w //= 2
    return s[0]


def add(tracks, frame_count, ids, pts, min_parallax=MIN_PARALLAX):
    """addFeatureCheckParallax with the device rules of include/vio_fm.h.  Returns (tracks, result); on a status the tracks come back
    unchanged."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    res = dict(status=STATUS_OK, keyframe=0, last_track_num=0, parallax_num=0, parallax_sum=0.0, parallax_sum_ref=0.0, n_new=0)
    new = copy_tracks(tracks)
    row = {t["id"]: i for i, t in enumerate(new)}
    err, last, n_new = 0, 0, 0
    for k in np.argsort(ids, kind="stable"):                  # the std::map's order
        fid = int(ids[k])
        if fid in row:
            t = new[row[fid]]
            if len(t["pts"]) >= MAX_OBS:
                err |= 4
            elif t["start"] + len(t["pts"]) != frame_count:
                err |= 2
            t["pts"] = np.vstack([t["pts"], pts[k]])
            last += 1
        else:
            new.append(dict(id=fid, start=int(frame_count), depth=-1.0, flag=0, pts=pts[k].reshape(1, 2).copy()))
            n_new += 1
    if len(tracks) + n_new > MAX_TRACKS:
        err |= 1
    if err:
        res["status"] = STATUS_TABLE_FULL if err & 1 else (STATUS_OBS_FULL if err & 4 else STATUS_GAP)
        return copy_tracks(tracks), dict(res, **dict(zip(("n_tracks", "n_landmarks", "n_observations"), counts(tracks))))
    res.update(last_track_num=last, n_new=n_new)
    res.update(zip(("n_tracks", "n_landmarks", "n_observations"), counts(new)))
    if frame_count < 2 or last < 20:
        res["keyframe"] = 1
        return new, res
    terms = parallax_terms(new, frame_count)
    num = sum(v is not None for v in terms)
    if num == 0:
        res["keyframe"] = 1
        return new, res
    res.update(parallax_num=num, parallax_sum=sum_device_order(terms), parallax_sum_ref=sum_reference_order(terms))
    res["keyframe"] = int(res["parallax_sum_ref"] / num >= min_parallax)
    return new, res


def set_depth(tracks, x, clear=False):
    new, k = copy_tracks(tracks), -1
    for t in new:
        if not usable(t):
            continue
        k += 1
        t["depth"] = 1.0 / float(x[k])
        if not clear:
            t["flag"] = 2 if t["depth"] < 0 else 1
    assert k + 1 == len(x)
    return new


def remove_failures(tracks):
    return [t for t in copy_tracks(tracks) if t["flag"] != 2]


def shift_depth(x, y, depth, mR, mP, nR, nP, init_depth=INIT_DEPTH):
    """csrc/vio_fm_math.h fm_shift_depth, operation for operation."""
    mR, nR = np.asarray(mR, dtype=np.float64).reshape(3, 3), np.asarray(nR, dtype=np.float64).reshape(3, 3)
    p = (float(x) * depth, float(y) * depth, 1.0 * depth)
    d = []
    for r in range(3):
        a, b, c = float(mR[r, 0]) * p[0], float(mR[r, 1]) * p[1], float(mR[r, 2]) * p[2]
        w = ((a + b) + c) + float(mP[r])
        d.append(w - float(nP[r]))
    a, b, c = float(nR[0, 2]) * d[0], float(nR[1, 2]) * d[1], float(nR[2, 2]) * d[2]
    dep = (a + b) + c
    return dep if dep > 0 else init_depth


def shift_depth_bound(x, y, depth, mR, mP, nR, nP):
    """8 * 2^-52 * (|new_R|^T (|marg_R| |pts_i| + |marg_P| + |new_P|))[2]: a forward error bound of the two matrix-vector products in
    either evaluation order."""
    mR, nR = np.abs(np.asarray(mR, dtype=np.float64).reshape(3, 3)), np.abs(np.asarray(nR, dtype=np.float64).reshape(3, 3))
    p = np.abs(np.array([x * depth, y * depth, depth]))
    return 8.0 * 2.0 ** -52 * float((nR.T @ (mR @ p + np.abs(mP) + np.abs(nP)))[2])


def slide_row(kind, frame_count, start, n_obs):
    """csrc/vio_fm_math.h fm_slide_row: (start, erase, keep, shift)."""
    if kind == FRONT:
        if start == frame_count:
            return start - 1, -1, 1, 0
        j = WINDOW_SIZE - 1 - start
        if start + n_obs - 1 < frame_count - 1 or j < 0 or j >= n_obs:
            return start, -1, 1, 0
        return start, j, int(n_obs - 1 != 0), 0
    if start != 0:
        return start - 1, -1, 1, 0
    if kind == BACK_SHIFT_DEPTH:
        keep = int(not n_obs - 1 < 2)
        return start, 0, keep, keep
    return start, 0, int(n_obs - 1 != 0), 0


def slide(tracks, kind, frame_count=0, marg_R=None, marg_P=None, new_R=None, new_P=None, init_depth=INIT_DEPTH):
    out = []
    for t in copy_tracks(tracks):
        start, erase, keep, shift = slide_row(kind, frame_count, t["start"], len(t["pts"]))
        if not keep:
            continue
        if shift:
            t["depth"] = shift_depth(t["pts"][0, 0], t["pts"][0, 1], t["depth"], marg_R, marg_P, new_R, new_P, init_depth)
        t["start"] = start
        if erase >= 0:
            t["pts"] = np.delete(t["pts"], erase, axis=0)
        out.append(t)
    return out


def corresponding(tracks, l, r):
    rows = [[t["pts"][l - t["start"], 0], t["pts"][l - t["start"], 1], t["pts"][r - t["start"], 0], t["pts"][r - t["start"], 1]]
            for t in tracks if t["start"] <= l and t["start"] + len(t["pts"]) - 1 >= r]
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def quat_to_rot(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def triangulate_track(t, Rc, tc, init_depth=INIT_DEPTH):
    """feature_manager.cpp:212-254 for one track; returns (depth, whether the < 0.1 fallback fired)."""
    s = t["start"]
    R0, t0 = Rc[s], tc[s]
    A = []
    for j, p in enumerate(t["pts"]):
        R1, t1 = Rc[s + j], tc[s + j]
        tt = R0.T @ (t1 - t0)
        R = R0.T @ R1
        P = np.hstack([R.T, (-R.T @ tt).reshape(3, 1)])
        f = np.array([p[0], p[1], 1.0])
        f = f / np.linalg.norm(f)
        A.append(f[0] * P[2] - f[2] * P[0])
        A.append(f[1] * P[2] - f[2] * P[1])
    v = np.linalg.svd(np.array(A))[2][-1]
    dep = v[2] / v[3]
    return (init_depth, True) if dep < 0.1 else (float(dep), False)


def triangulate(tracks, poses, ext, init_depth=INIT_DEPTH):
    """Returns (tracks, rows triangulated, rows where the fallback fired)."""
    poses, ext = np.asarray(poses, dtype=np.float64).reshape(11, 7), np.asarray(ext, dtype=np.float64).reshape(7)
    ric = quat_to_rot(ext[3:7])
    Rc = [quat_to_rot(poses[k, 3:7]) @ ric for k in range(11)]
    tc = [poses[k, 0:3] + quat_to_rot(poses[k, 3:7]) @ ext[0:3] for k in range(11)]
    new, done, fell = copy_tracks(tracks), [], []
    for i, t in enumerate(new):
        if not usable(t) or t["depth"] > 0:
            continue
        t["depth"], fb = triangulate_track(t, Rc, tc, init_depth)
        done.append(i)
        if fb:
            fell.append(i)
    return new, done, fell


def export(tracks):
    """getDepthVector and the edge loop of estimator.cpp:975-1016 over the tracks as they are."""
    ids, inv, lm, host, target, pi, pj = [], [], [], [], [], [], []
    for t in tracks:
        if not usable(t):
            continue
        k = len(ids)
        ids.append(t["id"])
        inv.append(1.0 / t["depth"])
        for j in range(1, len(t["pts"])):
            lm.append(k); host.append(t["start"]); target.append(t["start"] + j)
            pi.append(t["pts"][0]); pj.append(t["pts"][j])
    return dict(feature_ids=np.array(ids, dtype=np.int64), inv_depth=np.array(inv, dtype=np.float64), lm=np.array(lm, dtype=np.int32),
                host=np.array(host, dtype=np.int32), target=np.array(target, dtype=np.int32),
                pts_i=np.array(pi, dtype=np.float64).reshape(-1, 2), pts_j=np.array(pj, dtype=np.float64).reshape(-1, 2))


def apply_op(tracks, op, poses=None, ext=None):
    """One operation of tests/fm_util.py's codes."""
    c = op[0]
    if c == 1:
        return triangulate(tracks, poses, ext)[0]
    if c == 2:
        return set_depth(tracks, op[1])
    if c == 3:
        return remove_failures(tracks)
    if c == 4:
        return slide(tracks, BACK_SHIFT_DEPTH, 0, *op[1:5])
    if c == 5:
        return slide(tracks, BACK)
    if c == 6:
        return slide(tracks, FRONT, op[1])
    if c == 7:
        return set_depth(tracks, op[1], clear=True)
    raise ValueError(c)


def tracks_to_arrays(tracks):
    """The arguments of FmHandle.tracks_set."""
    off = np.concatenate([[0], np.cumsum([len(t["pts"]) for t in tracks])]).astype(np.int64)
    pts = np.concatenate([t["pts"].reshape(-1, 2) for t in tracks]) if tracks else np.zeros((0, 2))
    return (np.array([t["id"] for t in tracks], dtype=np.int64), np.array([t["start"] for t in tracks], dtype=np.int32),
            np.array([t["depth"] for t in tracks], dtype=np.float64), np.array([t.get("flag", 0) for t in tracks], dtype=np.int32), off, pts)


def arrays_to_tracks(d):
    off = d["off"]
    return [dict(id=int(d["ids"][i]), start=int(d["start"][i]), depth=float(d["depth"][i]), flag=int(d["flag"][i]),
                 pts=np.array(d["pts"][off[i]:off[i + 1]], dtype=np.float64)) for i in range(len(d["ids"]))]


def assert_tracks_equal(got, want):
    """Every field byte for byte, the depths included."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["id"], g["start"], g["flag"]) == (w["id"], w["start"], w["flag"]), (i, g, w)
        assert np.array_equal(g["pts"], w["pts"]), (i, g, w)
        assert np.float64(g["depth"]).tobytes() == np.float64(w["depth"]).tobytes(), (i, g["depth"], w["depth"])
