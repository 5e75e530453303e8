"""The numpy restatement of include/vio_aif.h: the reference Estimator's all_image_frame and tmp_pre_integration (estimator.cpp
:46-103, :107-138, :156-159, :1186-1199), operation for operation in the header's order.  It is the pin of libvio_aif_hip.so, which is
formally unpinned (the oracle does not compile the reference's Estimator).

A slot is a dict: frames (a list of dicts t, ids, pts, R, T, is_key and the frame's interval: exists, first, bias, dt, acc, gyr), open
(the open interval, tmp_pre_integration), acc_0, gyr_0, first_imu: what AifHandle.frames_get returns.  ImageFramesReference has the
batched methods of AifHandle, so BatchImageFrames runs over either.
"""
import numpy as np

MAX_SLOTS, MAX_FRAMES, MAX_FRAME_POINTS, MAX_POINTS, MAX_SAMPLES, OFFS = 256, 32, 1024, 8192, 4096, 34
STATUS_OK, STATUS_POOL_FULL, STATUS_FRAMES_FULL, STATUS_NO_FRAME, STATUS_WALK = 0, 1, 2, 3, 4
MAX_KEY, MAX_TRACKS = 32, 4096
DEFAULT_NOISE = (0.2687, 0.2121, 7.07e-6, 7.07e-7)
DEFAULT_MIN_POINTS = 6


def new_interval(exists=0, first=None, bias=None):
    return dict(exists=int(exists), first=np.zeros(6) if first is None else np.array(first, dtype=np.float64),
                bias=np.zeros(6) if bias is None else np.array(bias, dtype=np.float64), dt=np.zeros(0), acc=np.zeros((0, 3)), gyr=np.zeros((0, 3)))


def new_slot():
    return dict(frames=[], open=new_interval(), acc_0=np.zeros(3), gyr_0=np.zeros(3), first_imu=0)


def rank(ids, i):
    """aif_rank: the number of ids below ids[i]."""
    return int(sum(1 for v in ids if v < ids[i]))


def find(ts, t_0):
    """aif_find: the index of t_0 among the headers, or -1."""
    k = -1
    for j, t in enumerate(ts):
        if t == t_0:
            k = j
    return k


def imu_status(open_exists, held, n):
    return STATUS_POOL_FULL if open_exists and held + n > MAX_SAMPLES else STATUS_OK


def image_status(n_frames, held, n):
    if n_frames >= MAX_FRAMES:
        return STATUS_FRAMES_FULL
    return STATUS_POOL_FULL if held + n > MAX_POINTS else STATUS_OK


def slid_off(off, last, k, j):
    """aif_slid_off: entry j of the offsets after frames 0 .. k left."""
    return int(off[min(j + k + 1, last)] - off[k + 1] + off[0])


def n_samples(s):
    return sum(len(f["dt"]) for f in s["frames"]) + len(s["open"]["dt"])


def n_points(s):
    return sum(len(f["ids"]) for f in s["frames"])


def result(s, status=STATUS_OK, **kw):
    r = dict(status=status, n_frames=len(s["frames"]), n_points=n_points(s), n_samples=n_samples(s), erased_frames=0, erased_samples=0, records=0)
    r.update(kw)
    return r


def process_imu(s, dt, acc, gyr):
    """processIMU's part (:107-112, :122, :137-138) for a run of samples."""
    dt, acc, gyr = np.asarray(dt, dtype=np.float64).reshape(-1), np.asarray(acc, dtype=np.float64).reshape(-1, 3), np.asarray(gyr, dtype=np.float64).reshape(-1, 3)
    n, op = len(dt), s["open"]
    st = imu_status(op["exists"], n_samples(s), n)
    if st != STATUS_OK or n == 0:
        return result(s, st)
    s["first_imu"] = 1
    if op["exists"]:
        op["dt"], op["acc"], op["gyr"] = np.concatenate([op["dt"], dt]), np.concatenate([op["acc"], acc]), np.concatenate([op["gyr"], gyr])
    s["acc_0"], s["gyr_0"] = acc[-1].copy(), gyr[-1].copy()
    return result(s)


def process_image(s, t, ids, pts, ba, bg):
    """processImage's insert (:156-159)."""
    ids, pts = np.asarray(ids, dtype=np.int64).reshape(-1), np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    n = len(ids)
    if n > MAX_FRAME_POINTS or len(set(ids.tolist())) != n or not np.isfinite(t) or (s["frames"] and not t > s["frames"][-1]["t"]):
        raise ValueError("VIO_ERR_BAD_ARG")
    st = image_status(len(s["frames"]), n_points(s), n)
    if st != STATUS_OK:
        return result(s, st)
    sid, spt = np.zeros(n, dtype=np.int64), np.zeros((n, 2))
    ranks = (ids[None, :] < ids[:, None]).sum(axis=1)      # aif_rank of every point
    sid[ranks], spt[ranks] = ids, pts
    f = dict(t=float(t), ids=sid, pts=spt, R=np.zeros(9), T=np.zeros(3), is_key=0)
    f.update(s["open"])                             # imageframe.pre_integration = tmp_pre_integration
    s["frames"].append(f)
    s["open"] = new_interval(1, np.concatenate([s["acc_0"], s["gyr_0"]]), np.concatenate([np.asarray(ba, dtype=np.float64).reshape(3), np.asarray(bg, dtype=np.float64).reshape(3)]))
    return result(s)


def slide(s, t_0):
    """slideWindow's erase (:1186-1199): every frame with header <= t_0 leaves."""
    k = find([f["t"] for f in s["frames"]], t_0)
    if k < 0:
        return result(s, STATUS_NO_FRAME)
    gone = s["frames"][:k + 1]
    s["frames"] = s["frames"][k + 1:]
    return result(s, erased_frames=k + 1, erased_samples=sum(len(f["dt"]) for f in gone))


def reset(s):
    """clearState's part: acc_0 / gyr_0 stay."""
    s["frames"], s["open"], s["first_imu"] = [], new_interval(), 0


def intervals(s):
    """The intervals of frames 1 .. F - 1 as ImuHandle.load takes them."""
    return [dict(acc0=f["first"][0:3], gyr0=f["first"][3:6], dt=f["dt"], acc=f["acc"], gyr=f["gyr"]) for f in s["frames"][1:]]


def same_slot(a, b):
    """Two slot dicts, bit for bit (floats by their bytes)."""
    eq = lambda x, y: np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes()
    ival = lambda x, y: x["exists"] == y["exists"] and all(eq(np.asarray(x[k], dtype=np.float64), np.asarray(y[k], dtype=np.float64)) for k in ("first", "bias", "dt", "acc", "gyr"))
    if len(a["frames"]) != len(b["frames"]) or a["first_imu"] != b["first_imu"]:
        return False
    if not (eq(np.asarray(a["acc_0"], dtype=np.float64), np.asarray(b["acc_0"], dtype=np.float64)) and eq(np.asarray(a["gyr_0"], dtype=np.float64), np.asarray(b["gyr_0"], dtype=np.float64))):
        return False
    if not ival(a["open"], b["open"]):
        return False
    for f, g in zip(a["frames"], b["frames"]):
        if not (np.float64(f["t"]).tobytes() == np.float64(g["t"]).tobytes() and f["is_key"] == g["is_key"] and ival(f, g)):
            return False
        if not (eq(np.asarray(f["ids"], dtype=np.int64), np.asarray(g["ids"], dtype=np.int64)) and all(eq(np.asarray(f[k], dtype=np.float64), np.asarray(g[k], dtype=np.float64)) for k in ("pts", "R", "T"))):
            return False
    return True


# ---- initialStructure's frame work (estimator.cpp:243-270, :308-374) ----
def quat_to_rot(q):
    """aif_quat_to_rot: Eigen's toRotationMatrix on (w, x, y, z), not normalised; 9 floats, row-major."""
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def mul_rict(A, ric):
    """aif_mul_rict: A ric^T, every element (A_i0 ric_j0 + A_i1 ric_j1) + A_i2 ric_j2."""
    A, ric = [float(v) for v in A], [float(v) for v in np.asarray(ric).reshape(-1)]
    return [(A[3 * i] * ric[3 * j] + A[3 * i + 1] * ric[3 * j + 1]) + A[3 * i + 2] * ric[3 * j + 2] for i in range(3) for j in range(3)]


def excitation(records):
    """aif_excitation over the (n, 467) records of frames 1 .. F - 1: sum_dt at [0], delta_v at [8:11].  n = 0 gives NaN."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 467)
    n = len(rec)
    sum_g = [np.float64(0.0)] * 3
    with np.errstate(all="ignore"):                         # (a record with sum_dt 0, an interval without samples, divides 0 by 0)
        for r in rec:
            for c in range(3):
                sum_g[c] = sum_g[c] + r[8 + c] / r[0]
        dn = np.float64(n)
        aver = [np.float64(sum_g[c] * 1.0) / dn for c in range(3)]
        var = np.float64(0.0)
        for r in rec:
            x, y, z = (r[8 + c] / r[0] - aver[c] for c in range(3))
            var = var + ((x * x + y * y) + z * z)
        return float(np.sqrt(var / dn))


def walk(ts, headers):
    """aif_walk: (status, is_key, guess) of the key walk as written (:309-327)."""
    n_key, i, found = len(headers), 0, 0
    is_key, guess = [0] * len(ts), [0] * len(ts)
    for j, t in enumerate(ts):
        if i >= n_key:
            return STATUS_WALK, None, None
        if t == headers[i]:
            is_key[j], guess[j] = 1, i
            i += 1
            found += 1
            continue
        if t > headers[i]:
            i += 1
        if i >= n_key:
            return STATUS_WALK, None, None
        guess[j] = i
    if found != n_key:
        return STATUS_WALK, None, None
    return STATUS_OK, is_key, guess


def pnp_item(s, item, is_key, guess):
    """The vio_pnp item of a slot's non-keyframes: the observations in ascending id, ids the tracks do not list left out."""
    track = {int(v): k for k, v in enumerate(np.asarray(item["track_ids"]).reshape(-1).tolist())}
    off, op, ob, gk = [0], [], [], []
    for f, key, g in zip(s["frames"], is_key, guess):
        if key:
            continue
        for fid, p in zip(f["ids"].tolist(), f["pts"]):
            if fid in track:
                op.append(track[fid])
                ob.append(p)
        off.append(len(op))
        gk.append(g)
    return dict(points=np.asarray(item["points"], dtype=np.float64).reshape(-1, 3), valid=np.asarray(item["state"]).reshape(-1) != 0,
                key_Q=np.asarray(item["Q"], dtype=np.float64).reshape(-1, 4), key_T=np.asarray(item["T"], dtype=np.float64).reshape(-1, 3),
                guess_key=np.array(gk, dtype=np.int32), obs_offset=np.array(off, dtype=np.int64), obs_point=np.array(op, dtype=np.int32),
                obs_pts=np.array(ob, dtype=np.float64).reshape(-1, 2))


def finish(s, item, is_key, guess, pnp):
    """R (F, 9), T (F, 3) of every frame (:316-320, :365-373) from the SfM's keyframes and a vio_pnp result dict of pnp_item's item; the
    rows go into the slot's frames too.  A failed frame is NaN; a window that is not finite is NaN in every non-keyframe."""
    F = len(s["frames"])
    R, T, m = np.full((F, 9), np.nan), np.full((F, 3), np.nan), 0
    bad = pnp["status"] == -3
    for j in range(F):
        if is_key[j]:
            R[j], T[j] = mul_rict(quat_to_rot(item["Q"][guess[j]]), item["ric"]), np.asarray(item["T"][guess[j]], dtype=np.float64)
        else:
            if not bad and pnp["frame_status"][m] == 0:
                R[j], T[j] = mul_rict(quat_to_rot(pnp["Q"][m]), item["ric"]), pnp["T"][m]
            m += 1
        s["frames"][j].update(R=R[j].copy(), T=T[j].copy(), is_key=int(is_key[j]))
    return R, T


class ImageFramesReference:
    """The batched methods of AifHandle over slot dicts."""

    def __init__(self):
        self.slots = {}

    def slot(self, s):
        return self.slots.setdefault(int(s), new_slot())

    def reset(self, slot):
        reset(self.slot(slot))

    def frames_get(self, slot):
        return self.slot(slot)

    def imu_batch(self, items):
        return [process_imu(self.slot(s), dt, acc, gyr) for s, dt, acc, gyr in items]

    def image_batch(self, items):
        return [process_image(self.slot(s), t, ids, pts, ba, bg) for s, t, ids, pts, ba, bg in items]

    def slide_batch(self, items):
        return [slide(self.slot(s), t_0) for s, t_0 in items]
