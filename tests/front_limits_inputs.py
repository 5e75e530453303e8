"""The inputs of the front end's tests at full tables (tests/test_front_limits_inputs_cpu.py holds them to the numpy restatements,
tests/test_gpu_front_limits.py and tests/test_gpu_detect_limits.py run them on the device).  No tests in here.

    image(t, seed)          frame t of a 192 x 144 stream: frame_sequences.image, and from frame 1 on the 24 x 24 blocks with
                            ((y // 24) + (x // 24)) % 4 == 0 hold the same texture moving another way, so that rejectWithF has real
                            outliers and its mask is mixed
    CAM, RANSAC             a camera for that geometry (tests/test_gpu_front.py's, scaled) and the RANSAC settings of that file
    corners(seed)           every corner the numpy detector finds on frame 0 at min_distance 1, strongest first
    seeded(n, seed)         the first n of them with distinct ids and track_cnt = k % 5 + 2 (setMask's keep_order is a real permutation)
    strong(n)               the first n corners at least 11 pixels from every edge
    margin_points(n)        n positions at x = 3: inside a border margin of 8, where they stay whichever way the texture moves
    waves_with_drops(keep)  the wavefronts (rows 64 w .. 64 w + 63) of a keep mask that drop at least one row

A 64 x 48 frame yields about 150 corners; this geometry yields more than 1024 at min_distance <= 2, which is what fills a slot's table.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as flow_ref  # noqa: E402
import frame_sequences as fs  # noqa: E402

W, H = 192, 144
CAP, WAVE = 1024, 64                                # a slot's table and a wavefront of it
SEED = 5
BLOCK, PLANTED_SHIFT = 24, (-1.5, -2.5)
CAM = dict(fx=156.0, fy=153.0, cx=95.5, cy=71.6, k1=-0.12, k2=0.02, p1=3e-4, p2=-2e-4, width=W, height=H)
RANSAC = dict(seed=3, ransac_hypotheses=128, f_threshold=1.0, focal_length=460.0)
FLOW = dict(levels=2, half_patch=2)
MIN_DIST, BORDER, DT = 2, 1, 0.05
ID0 = 10000                                         # the seeded rows' first id: apart from the ids a slot's counter gives
_cache = {}


def planted():
    """True where the texture moves by PLANTED_SHIFT a frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy // BLOCK) + (xx // BLOCK)) % 4 == 0


def image(t, seed=SEED):
    key = ("image", seed, t)
    if key not in _cache:
        img = np.ascontiguousarray(fs.image(W, H, seed, t)).copy()
        if t > 0:
            other = flow_ref.texture(W, H, seed=seed, shift=(PLANTED_SHIFT[0] * t, PLANTED_SHIFT[1] * t), smooth=1.5)
            img[planted()] = other[planted()]
        if t % 3 == 2:                              # rows of another stride than the width, as frame_sequences.image has them
            wide = np.full((H, W + 5), 255, dtype=np.uint8)
            wide[:, :W] = img
            img = wide[:, :W]
        _cache[key] = img
    return _cache[key]


def corners(seed=SEED):
    key = ("corners", seed)
    if key not in _cache:
        _cache[key] = dr.detect(np.ascontiguousarray(image(0, seed)), max_total=4096, min_distance=1)["new_pts"].astype(np.float32)
    return _cache[key]


def seeded(n, seed=SEED):
    """(pts (n, 2) float32, ids (n,) int64, track_cnt (n,) int32)."""
    p = corners(seed)
    assert len(p) >= n, (len(p), n)
    k = np.arange(n)
    return p[:n].copy(), (ID0 + k).astype(np.int64), (k % 5 + 2).astype(np.int32)


def inner(pts, margin):
    """The rows of pts at least `margin` pixels from every edge."""
    p = np.asarray(pts)
    return (p[:, 0] >= margin) & (p[:, 0] < W - margin) & (p[:, 1] >= margin) & (p[:, 1] < H - margin)


def strong(n, margin=11, seed=SEED):
    """The first n corners at least `margin` pixels from every edge: they track and stay inside a border of 8."""
    p = corners(seed)
    p = p[inner(p, margin)]
    assert len(p) >= n, (len(p), n)
    return p[:n].copy()


def margin_points(n):
    y = 10.0 + np.arange(n) * ((H - 20.0) / max(n, 1))
    return np.stack([np.full(n, 3.0), y], axis=1).astype(np.float32)


def waves_with_drops(keep):
    keep = np.asarray(keep, dtype=bool)
    return sorted(set((np.nonzero(~keep)[0] // WAVE).tolist()))
