"""Synthetic initialisation windows for the tests of vio_aif_structure_batch: frames on a smooth path, the SfM's keyframe poses and
points as ground truth, every frame's observations as exact projections, and between the frames the raw IMU samples of a body that
carries the camera along that path (the path differentiated, with gravity, a gyro bias and a little noise), so that the visual-inertial
alignment of a window succeeds.  The patterns put non-keyframes at the front, in the middle and two in a row;
tests/test_aif_reference.py checks on the CPU that tests/pnp_reference.py alone solves every non-keyframe of every scene used on the
device, and that tests/init_reference.py alone aligns the windows of the end-to-end test."""
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
