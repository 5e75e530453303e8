"""Synthetic initialisation windows for the tests of vio_aif_structure_batch: frames on a smooth path, the SfM's keyframe poses and
points as ground truth, every frame's observations as exact projections, and between the frames the raw IMU samples of a body that
carries the camera along that path (the path differentiated, with gravity, a gyro bias and a little noise), so that the visual-inertial
alignment of a window succeeds.  The patterns put non-keyframes at the front, in the middle and two in a row;
tests/test_aif_reference.py checks on the CPU that tests/pnp_reference.py alone solves every non-keyframe of every scene used on the
device, and that tests/init_reference.py alone aligns the windows of the end-to-end test.  build() makes scenes of any shape for
tests/test_gpu_aif_limits.py (LIMIT_SCENES): any pattern, up to 4096 tracks with ids that are negative, above 2^32 and unordered, any
number of observations per frame with the unusable ones at chosen positions of the stored order, intervals without samples, a body at
rest; make() and its scenes are as they were."""
import numpy as np

import aif_reference as ar

PATTERNS = {                                            # k: keyframe, n: non-keyframe; 11 keyframes each
    "front": "nk" + "k" * 10,                           # 12 frames: a leading non-keyframe
    "middle": "kknkkknnkkkknkk",                        # 15 frames: one, two in a row, one
    "full": "nnk" * 10 + "nk",                          # 32 frames: the most a slot holds
}
RIC = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[0.98, 0.0, 0.198997487421324], [0.0, 1.0, 0.0], [-0.198997487421324, 0.0, 0.98]])
TIC = np.array([0.02, -0.01, 0.03])                     # the camera in the body
SCALE = 2.0                                             # metres per unit of the SfM's frame
GRAVITY = 9.81 * np.array([0.6, -0.64, 0.48])           # in the SfM's frame
BG_TRUE = np.array([0.004, -0.003, 0.002])              # the gyroscope's bias
FRAME_DT = 0.1
AXIS = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])


def pose(j, rng_off=0.0):
    """The camera in the SfM's frame at frame j (any real j): q (w, x, y, z) and the position."""
    a = 0.015 * j + rng_off
    q = np.concatenate([[np.cos(a / 2)], AXIS * np.sin(a / 2)])
    return q, np.array([0.12 * j, 0.03 * np.sin(0.7 * j), 0.01 * j])


def imu(j):
    """What an ideal IMU reads at frame time j (any real j): the body's rotation is R_c RIC^T, its position SCALE p_c - R_b TIC in
    metres, and acc = R_b^T (p_b'' + GRAVITY), gyr = the body's rate + BG_TRUE.  The camera turns about a fixed axis at a constant rate,
    so the body's rate is the constant w = RIC AXIS da/dt and R_b'' TIC = R_b (w x (w x TIC))."""
    q, _ = pose(j)
    Rb = np.array(ar.quat_to_rot(q)).reshape(3, 3) @ RIC.T
    w = RIC @ AXIS * (0.015 / FRAME_DT)
    pc_dd = np.array([0.0, -0.03 * 0.49 * np.sin(0.7 * j), 0.0]) / (FRAME_DT * FRAME_DT)
    a = SCALE * pc_dd - Rb @ np.cross(w, np.cross(w, TIC))
    return Rb.T @ (a + GRAVITY), w + BG_TRUE


def make(pattern, seed, n_tracks=40, seen=0.8, strangers=3, dead=4, n_smp=20):
    """A scene: frames (t, ids, pts, samples, ba, bg per frame, shuffled ids), and the structure item without its slot."""
    rng = np.random.RandomState(seed)
    pat = PATTERNS[pattern]
    assert pat.count("k") == 11
    X = np.stack([rng.uniform(-2.5, 3.5, n_tracks), rng.uniform(-2, 2, n_tracks), rng.uniform(4, 8, n_tracks)], axis=1)
    track_ids = rng.choice(100000, n_tracks, replace=False).astype(np.int64) - 500
    state = np.ones(n_tracks, dtype=np.uint8)
    state[rng.choice(n_tracks, dead, replace=False)] = 0
    frames, Q, T, headers = [], [], [], []
    for j, c in enumerate(pat):
        q, p = pose(j)
        R = np.array(ar.quat_to_rot(q)).reshape(3, 3)
        Xc = (X - p) @ R
        see = np.nonzero(rng.uniform(size=n_tracks) < seen)[0]
        ids = np.concatenate([track_ids[see], 200000 + rng.choice(1000, strangers, replace=False)])      # ... and ids no track has
        pts = np.concatenate([Xc[see, :2] / Xc[see, 2:3], rng.uniform(-0.5, 0.5, (strangers, 2))])
        order = rng.permutation(len(ids))
        t = 100.0 + FRAME_DT * j
        ba, bg = rng.randn(3) * 0.02, rng.randn(3) * 0.002                                             # the interval's constructor biases
        ideal = [imu(j - 1 + (k + 1) / n_smp) for k in range(n_smp)]                                    # the last sample is at the image
        acc = np.array([a for a, _ in ideal]) + rng.randn(n_smp, 3) * 0.01
        gyr = np.array([g for _, g in ideal]) + rng.randn(n_smp, 3) * 0.001
        frames.append(dict(t=t, ids=ids[order], pts=pts[order], ba=ba, bg=bg, samples=(np.full(n_smp, FRAME_DT / n_smp), acc, gyr)))
        if c == "k":
            Q.append(q); T.append(p); headers.append(t)
    points = X.copy()
    points[state == 0] = np.nan                         # as vio_sfm_construct_batch leaves them
    item = dict(headers=np.array(headers), Q=np.array(Q), T=np.array(T), track_ids=track_ids, points=points, state=state, ric=RIC)
    return dict(frames=frames, item=item, is_key=[int(c == "k") for c in pat])


ID_STEP = 4096                                          # build()'s track ids are multiples of it: every gap holds strangers
REST_ACC, REST_GYR = np.array([0.3, -0.2, 9.78]), np.array([0.001, -0.002, 0.0005])      # what build(rest=True)'s IMU reads, always


def _per_frame(v, pat, what):
    """One number per frame from one number, a (keyframes, non-keyframes) tuple or a list of len(pat)."""
    if np.ndim(v) == 0:
        return [int(v)] * len(pat)
    if isinstance(v, tuple):
        return [int(v[0] if c == "k" else v[1]) for c in pat]
    assert len(v) == len(pat), what
    return [int(x) for x in v]


def build(pattern, seed, n_tracks, n_seen, strangers=3, dead=0, n_smp=20, bad_at=None, dead_sorted=None, rest=False):
    """A scene as make()'s, of any shape.  pattern: a key of PATTERNS or any string of k / n; n_seen: the tracks a frame sees, one number,
    a (keyframes, non-keyframes) tuple or a list with one per frame; strangers: ids no track has, per frame (likewise); dead: the number of tracks with
    state 0, or dead_sorted: their positions in the id-sorted track table; n_smp: samples per interval, one number or one per frame,
    0 allowed; rest: a body at rest (constant acc and gyr, zero constructor biases).

    The track ids are distinct multiples of ID_STEP, some negative and some above 2^32, in random order.  A frame that sees two tracks
    or more sees the smallest and the largest id; its strangers lie, in this order, between two neighbours of the sorted table, below
    the smallest id and above the largest, then between neighbours again.

    bad_at: {frame: stored positions} (negative: from the end).  Such a frame has n_seen + strangers stored observations as well, but
    of them exactly those at the given positions of its stored (ascending id) order are unusable, alternately a stranger and, where
    one lies in the gap, a dead track; all others are live tracks, the smallest and the largest live id among them."""
    rng = np.random.RandomState(seed)
    pat = PATTERNS.get(pattern, pattern)
    assert pat and set(pat) <= {"k", "n"} and 1 <= pat.count("k") <= 32 and len(pat) <= 32
    seen_n, str_n, smp_n = _per_frame(n_seen, pat, "n_seen"), _per_frame(strangers, pat, "strangers"), _per_frame(n_smp, pat, "n_smp")
    X = np.stack([rng.uniform(-2.5, 3.5, n_tracks), rng.uniform(-2, 2, n_tracks), rng.uniform(4, 8, n_tracks)], axis=1)
    track_ids = (rng.choice(1 << 21, n_tracks, replace=False).astype(np.int64) - (1 << 20)) * ID_STEP
    track_ids[rng.uniform(size=n_tracks) < 0.3] += 1 << 33
    by_id = np.argsort(track_ids)                       # by_id[r]: the track at position r of the sorted table
    state = np.ones(n_tracks, dtype=np.uint8)
    if dead_sorted is not None:
        state[by_id[list(dead_sorted)]] = 0
    else:
        state[rng.choice(by_id[1:-1] if bad_at else n_tracks, dead, replace=False)] = 0      # (with bad_at the table's ends are live: seen and usable)
    lo_id, hi_id = (int(track_ids.min()), int(track_ids.max())) if n_tracks else (0, 0)
    bad_at = bad_at or {}

    def plain(n_see, n_str):
        """The tracks and stranger ids of a frame without bad_at."""
        assert n_see <= n_tracks
        must = [int(by_id[0]), int(by_id[-1])] if n_see >= 2 else []
        if dead_sorted is not None and n_see >= len(dead_sorted) + 2:      # the tracks named dead are seen
            must += [int(k) for k in by_id[list(dead_sorted)] if int(k) not in must]
        others = np.setdiff1d(np.arange(n_tracks), must)
        see = np.concatenate([must, rng.choice(others, n_see - len(must), replace=False)]).astype(np.int64)
        out = []
        for k in range(n_str):
            if n_tracks == 0:
                out.append(7 + 3 * k)
            elif k == 1:
                out.append(lo_id - 5)
            elif k == 2:
                out.append(hi_id + 5)
            else:
                out.append(int(track_ids[by_id[rng.randint(0, max(n_tracks - 1, 1))]]) + 1 + k)      # (not above the largest id)
        return see, np.array(out, dtype=np.int64)

    def placed(n_obs, where):
        """The tracks and stranger ids of a frame whose unusable observations sit at the stored positions `where`.  The stored order
        is written down first, position by position: usable, or unusable as a stranger and a dead track in turn.  Then one pass up
        the sorted table fills it: a usable position takes the next live row (the last one the last live row, the table's end), a
        dead one the next dead row if the live rows in front of it can be spared, and a stranger, or a dead position that found no
        row, an id just above the entry in front of it (the table's ids are ID_STEP apart), below the table at the front and above
        it behind the last usable position.  build() checks the outcome against `where`."""
        bad = sorted(set(p % n_obs for p in where))
        want = ["usable"] * n_obs
        for k, p in enumerate(bad):
            want[p] = "dead" if k % 2 else "stranger"
        is_live = state[by_id] != 0                     # the sorted table
        n_good = n_obs - len(bad)
        assert n_good <= is_live.sum() and len(bad) < ID_STEP
        see, strange, row, goods, prev, run, front, behind = [], [], 0, 0, None, 0, 0, 0
        for kind in want:
            nxt = None
            if kind == "usable":
                goods += 1
                nxt = int(np.nonzero(is_live)[0][-1]) if goods == n_good >= 2 else row + int(np.argmax(is_live[row:]))
            elif kind == "dead" and not is_live[row:].all():
                nxt = row + int(np.argmin(is_live[row:]))
                spared = int(is_live[row:nxt].sum())
                if int(is_live[nxt:].sum()) < n_good - goods or (spared and goods == 0 and n_good >= 2):
                    nxt = None                          # (the usable positions behind need those rows, or the first one the table's first)
            if nxt is None:
                run, front, behind = run + 1, front + (prev is None), behind + (goods == n_good and prev is not None)
                strange.append(lo_id - front if prev is None else hi_id + behind if goods == n_good else prev + run)
                continue
            see.append(int(by_id[nxt]))
            row, prev, run = nxt + 1, int(track_ids[by_id[nxt]]), 0
        return np.array(see, dtype=np.int64), np.array(strange, dtype=np.int64)

    frames, Q, T, headers = [], [], [], []
    for j, c in enumerate(pat):
        q, p = pose(j)
        R = np.array(ar.quat_to_rot(q)).reshape(3, 3)
        Xc = (X - p) @ R
        see, strange = placed(seen_n[j] + str_n[j], bad_at[j]) if j in bad_at else plain(seen_n[j], str_n[j])
        ids = np.concatenate([track_ids[see], strange]).astype(np.int64)
        assert len(set(ids.tolist())) == len(ids) == seen_n[j] + str_n[j]
        if j in bad_at:                                 # the unusable observations are where they were asked for
            live_ids = track_ids[state != 0]
            assert np.nonzero(~np.isin(np.sort(ids), live_ids))[0].tolist() == sorted(set(p % len(ids) for p in bad_at[j]))
        pts = np.concatenate([(Xc[see, :2] / Xc[see, 2:3]).reshape(-1, 2), rng.uniform(-0.5, 0.5, (len(strange), 2))])
        order = rng.permutation(len(ids))
        t = 100.0 + FRAME_DT * j
        rj, n = np.random.RandomState(1000 * seed + j), smp_n[j]           # (its own stream: another n_smp moves no other frame)
        if rest:
            ba, bg, acc, gyr = np.zeros(3), np.zeros(3), np.tile(REST_ACC, (n, 1)), np.tile(REST_GYR, (n, 1))
        else:
            ba, bg = rj.randn(3) * 0.02, rj.randn(3) * 0.002
            ideal = [imu(j - 1 + (k + 1) / n) for k in range(n)]
            acc = np.array([a for a, _ in ideal]).reshape(n, 3) + rj.randn(n, 3) * 0.01
            gyr = np.array([g for _, g in ideal]).reshape(n, 3) + rj.randn(n, 3) * 0.001
        frames.append(dict(t=t, ids=ids[order], pts=pts[order], ba=ba, bg=bg, samples=(np.full(n, FRAME_DT / max(n, 1)), acc, gyr)))
        if c == "k":
            Q.append(q); T.append(p); headers.append(t)
    points = X.copy()
    points[state == 0] = np.nan
    item = dict(headers=np.array(headers), Q=np.array(Q).reshape(-1, 4), T=np.array(T).reshape(-1, 3), track_ids=track_ids, points=points, state=state, ric=RIC)
    return dict(frames=frames, item=item, is_key=[int(c == "k") for c in pat])


def part(scene, lo, hi):
    """Frames lo .. hi - 1 of a scene, with the SfM of the keyframes among them."""
    k0, k1, item = sum(scene["is_key"][:lo]), sum(scene["is_key"][:hi]), scene["item"]
    return dict(frames=scene["frames"][lo:hi], is_key=scene["is_key"][lo:hi],
                item=dict(item, headers=item["headers"][k0:k1], Q=item["Q"][k0:k1], T=item["T"][k0:k1]))


def usable_counts(scene):
    """Per frame the stored observations whose id is a track with state != 0, in plain numpy from the ids."""
    item = scene["item"]
    ok = item["track_ids"][np.asarray(item["state"]) != 0]
    return [int(np.isin(f["ids"], ok).sum()) for f in scene["frames"]]


def unusable_positions(scene, frame):
    """The stored (ascending id) positions of `frame`'s unusable observations."""
    item = scene["item"]
    ok = item["track_ids"][np.asarray(item["state"]) != 0]
    return np.nonzero(~np.isin(np.sort(scene["frames"][frame]["ids"]), ok))[0].tolist()


# ---- the scenes of tests/test_gpu_aif_limits.py; tests/test_aif_reference.py checks on the CPU what each is meant to do ----
SIZES_PATTERN = "k" + "nk" * 10                         # ten non-keyframes, frames 1, 3, .. 19
SIZES = (0, 5, 6, 63, 64, 65, 255, 256, 257, 1024)      # their stored observations: 1995 in all
SIZES_BAD = (0, 63, 64, 255, 256)                       # where their unusable observations sit, and at the last position
POOL_PATTERN = "k" + "nk" * 8 + "kk"                    # 19 frames


def _sizes():
    seen, strangers, bad = [12] * 21, [3] * 21, {}
    for k, n in enumerate(SIZES):
        j = 2 * k + 1
        where = sorted(set([p for p in SIZES_BAD if p < n] + [n - 1])) if n >= 63 else []
        seen[j], strangers[j] = n - len(where), len(where)          # (with bad_at only the sum counts)
        bad[j] = where                                  # (an empty list: every observation is a live track)
    return build(SIZES_PATTERN, 51, 1200, seen, strangers, dead=100, bad_at=bad)


def _few_of_many(pattern, seed, usable, n_obs=1024, n_tracks=1200, dead=100):
    """Frames 1, 2, ..: n_obs stored observations each, of which usable[k] are usable, spread over the stored order."""
    seen, strangers, bad = [12] * len(pattern), [3] * len(pattern), {}
    for k, u in enumerate(usable):
        good = set(np.linspace(1, n_obs - 2, u).astype(int).tolist())
        assert len(good) == u
        seen[1 + k], strangers[1 + k], bad[1 + k] = u, n_obs - u, [p for p in range(n_obs) if p not in good]
    return build(pattern, seed, n_tracks, seen, strangers, dead=dead, bad_at=bad)


def _pool():
    seen = [12 if c == "k" else 1000 for c in POOL_PATTERN]
    seen[-1] += 3                                       # 8189 + 3: the pool is full
    return build(POOL_PATTERN, 42, 4096, seen, dead=300)


LIMIT_SCENES = {
    "tracks0": lambda: build("nkk", 30, 0, 0),
    "tracks1": lambda: build("nkk", 31, 1, 1),
    "tracks255": lambda: build("nkk", 33, 255, (12, 255), dead=4),          # the non-keyframe sees every track: every row of the table is looked up
    "tracks256": lambda: build("nkk", 34, 256, (12, 256), dead=4),
    "tracks257": lambda: build("nkk", 35, 257, (12, 257), dead=4),
    "tracks4096": lambda: build("nkk", 41, 4096, (12, 1021), dead_sorted=(0, 255, 256, 4095)),
    "sizes": _sizes,
    "five_six_of_1024": lambda: _few_of_many("knnk", 52, (5, 6)),
    "nkk257": lambda: build("nkk", 43, 257, (12, 62), dead=4),
    "pool": _pool,
    "one": lambda: build("k", 60, 40, 30, dead=4),
    "two": lambda: build("nk", 61, 40, 30, dead=4),
    "all_key": lambda: build("k" * 32, 62, 40, 30, dead=4, n_smp=5),
    "gap": lambda: build("front", 63, 40, 30, dead=4, n_smp=[20] * 5 + [0] + [20] * 6),
    "no_gap": lambda: build("front", 63, 40, 30, dead=4),
    "rest": lambda: build("front", 64, 40, 30, dead=4, rest=True),
    "nineteen_twenty": lambda: _few_of_many("knnk", 65, (19, 20), n_obs=23, n_tracks=40, dead=4),
    "longer": lambda: build(PATTERNS["middle"] + "knk", 66, 40, 30, dead=4),
}
_SCENES = {}


def limit_scene(name):
    """The named scene, built once; do not change it."""
    if name not in _SCENES:
        _SCENES[name] = LIMIT_SCENES[name]()
    return _SCENES[name]


def feed(handle, slot, scene):
    """The scene's samples and images into `slot` of an AifHandle or an ImageFramesReference."""
    for f in scene["frames"]:
        handle.imu_batch([(slot,) + f["samples"]])
        handle.image_batch([(slot, f["t"], f["ids"], f["pts"], f["ba"], f["bg"])])


def thin(scene, frame, keep):
    """The scene with `frame` seeing only `keep` of the usable tracks (and its strangers)."""
    item = scene["item"]
    ok = set(item["track_ids"][item["state"] != 0].tolist())
    f = scene["frames"][frame]
    usable = [k for k, v in enumerate(f["ids"].tolist()) if v in ok]
    drop = set(usable[keep:])
    sel = np.array([k for k in range(len(f["ids"])) if k not in drop])
    out = dict(scene, frames=list(scene["frames"]))
    out["frames"][frame] = dict(f, ids=f["ids"][sel], pts=f["pts"][sel])
    return out
