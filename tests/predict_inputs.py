"""The track tables, poses and cases of the prediction tests (tests/test_gpu_fm_predict.py, tests/test_fm_predict_cpu.py);
tests/test_predict_inputs_cpu.py asserts what the GPU file assumes of them.  A table is FmHandle.tracks_set's arrays: ids, start,
depth, flag, off, pts.

A row of a mixed table is drawn from four kinds: one that qualifies (depth > 0, n_obs >= 2, ends at frame_count), and one that fails
exactly one of the three conditions: the depth (-1, 0), the observation count (a single observation at frame_count), the end frame (ends
before frame_count or, where the window has room, behind it).  Some qualifying rows carry a denormal depth."""
import numpy as np

WINDOW, MAX_OBS, MAX_TRACKS = 10, 11, 2048
QUALIFIES, FAIL_DEPTH, FAIL_NOBS, FAIL_END = 0, 1, 2, 3
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048)
FRAME_COUNTS = (0, 1, 2, 10)


def poses(seed=0):
    """(poses (11, 7), ext (7,), next_pose (7,)): a smooth trajectory with unit quaternions (x, y, z, w), an extrinsic, a next pose that
    is not the constant-velocity one."""
    rng = np.random.RandomState(500 + seed)

    def quat(w):
        a = np.linalg.norm(w)
        q = np.concatenate([np.sin(a / 2) * w / a, [np.cos(a / 2)]])
        return q / np.linalg.norm(q)
    out = np.zeros((11, 7))
    v = rng.uniform(-0.3, 0.3, 3)
    w0 = rng.uniform(-0.2, 0.2, 3)
    for k in range(11):
        out[k, 0:3] = v * k + 0.02 * rng.normal(size=3)
        out[k, 3:7] = quat(w0 + 0.03 * k * np.array([0.5, -1.0, 0.8]) + 0.005 * rng.normal(size=3))
    ext = np.concatenate([[0.05, -0.02, 0.01], quat(np.array([0.01, -0.02, 0.015]))])
    nxt = np.concatenate([out[10, 0:3] + v * 1.3 + 0.01, quat(w0 + 0.36 * np.array([0.5, -1.0, 0.8]))])
    return out, ext, nxt


def kinds_of(n, frame_count, seed, share=0.6):
    """The kind of every row of a mixed table: `share` of them qualify, the rest fail one condition each, every kind present from
    four rows on; in a table of MAX_TRACKS rows the rows 64 .. 127 all qualify and the rows 128 .. 191 all fail."""
    rng = np.random.RandomState(9000 + 17 * n + frame_count + 1000 * seed)
    k = np.where(rng.uniform(size=n) < share, QUALIFIES, rng.randint(1, 4, size=n))
    if n >= 4:
        k[rng.choice(n, 4, replace=False)] = [QUALIFIES, FAIL_DEPTH, FAIL_NOBS, FAIL_END]
    if n == MAX_TRACKS:
        k[64:128] = QUALIFIES
        k[128:192] = rng.randint(1, 4, size=64)
    return k


def table(n, frame_count, seed=0, kinds=None):
    """A table of n rows around frame_count (in [1, 10]) and its kinds."""
    assert 1 <= frame_count <= WINDOW and 0 <= n <= MAX_TRACKS
    rng = np.random.RandomState(7000 + 13 * n + frame_count + 1000 * seed)
    fc = frame_count
    kinds = kinds_of(n, fc, seed) if kinds is None else np.asarray(kinds)
    ids = rng.choice(np.arange(-5000, 60000, dtype=np.int64), size=n, replace=False)
    if n >= 2:
        ids[0], ids[-1] = 2 ** 62 + 5, -2 ** 62 - 7
    start, nobs, depth = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
    for i, k in enumerate(kinds):
        K = int(rng.randint(2, fc + 2))                     # n_obs in [2, fc + 1]: the row ends at fc
        s = fc - K + 1
        d = float(rng.uniform(0.4, 30.0))
        if k == QUALIFIES and rng.uniform() < 0.05:
            d = float(rng.choice([5e-324, 1e-310, 2.2250738585072014e-308]))
        if k == FAIL_DEPTH:
            d = float(rng.choice([-1.0, 0.0, -0.0, -3.5]))
        elif k == FAIL_NOBS:
            K, s = 1, fc
        elif k == FAIL_END:
            if fc < WINDOW and (fc < 2 or rng.uniform() < 0.3):
                K = int(rng.randint(2, fc + 3))             # ends at fc + 1
                s = fc + 2 - K
            else:
                K = int(rng.randint(2, fc + 1))             # ends before fc
                s = int(rng.randint(0, fc - K + 1))
        start[i], nobs[i], depth[i] = s, K, d
    off = np.concatenate([[0], np.cumsum(nobs)]).astype(np.int64)
    pts = rng.uniform(-0.6, 0.6, (int(off[-1]), 2))
    return dict(ids=ids, start=start, depth=depth, flag=np.zeros(n, dtype=np.int32), off=off, pts=pts), kinds


def all_or_none(n, frame_count, every, seed=3):
    """A table where every row qualifies (every=True) or none does."""
    rng = np.random.RandomState(seed)
    kinds = np.zeros(n, dtype=np.int64) if every else rng.randint(1, 4, size=n)
    return table(n, frame_count, seed, kinds)[0]


def edge_depths(frame_count=5):
    """Six rows ending at frame_count with depths -1, 0, -0, a denormal, the smallest normal and 1: the last three qualify."""
    t, _ = table(6, frame_count, 11, np.zeros(6, dtype=np.int64))
    t["depth"] = np.array([-1.0, 0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.0])
    return t


# the mixed cases of the GPU file: every size at frame_count 10, and 65 and 1025 rows at the small frame counts
MIXED = [(n, 10) for n in SIZES if n >= 63] + [(65, 2), (1025, 2), (65, 5)]
# six slots of different sizes in one call: (slot, rows, frame_count)
SIX = [(3, 0, 10), (200, 1, 10), (7, 65, 2), (255, 1025, 10), (0, 2048, 10), (31, 64, 5)]
