"""Writes tests/golden/fm_large.npz: one addFeatureCheckParallax sequence at the size of a real front end, recorded from the compiled
reference's FeatureManager (oracle/_ref/libvio_ref.so: VM/src/feature_manager.cpp, driven by oracle/ref_feature_manager.cpp), so that
libvio_fm_hip (include/vio_fm.h) has a reference-pinned case beyond the 160 tracks of feature_manager.npz on a machine without the
reference.

    python tests/golden/make_golden_fm.py          (where oracle/_ref exists)

14 frames (frame_count 0 .. 10, then three more at 10) of 600 points, the ids of a frame shuffled, slides at frame_count == 10 as
Estimator::slideWindow does them (removeBack on a keyframe, removeFront otherwise).  The reference's ids are ints; what it does
depends on their order and equality alone, so it is driven with small ids and the file records id * ID_SCALE + ID_SHIFT, a monotonic
map that puts most of them above 2^31.  Asserted here: both decisions occur, and on every decided frame the mean parallax in the
reference's order is at least 1e-6 (relative) away from MIN_PARALLAX; two summation orders over n non-negative terms differ by at
most 2 (n - 1) 2^-53 of the sum, so no decision of the file can hinge on the order.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import fm_reference as fr      # noqa: E402
import fm_util as fu           # noqa: E402

ID_SCALE, ID_SHIFT = 3000011, 5


def random_rotation(rng):
    q = rng.normal(size=4)
    return fr.quat_to_rot(q / np.linalg.norm(q))


def make_frames(seed, n_frames=14, n_points=600, big_ids=True, survive=0.9):
    """[(frame_count, ids (n,), pts (n, 2))]: tracked points that move by a step whose size changes from frame to frame (so that the
    mean parallax falls on both sides of MIN_PARALLAX), a tenth of them lost and replaced per frame, the rows shuffled."""
    rng = np.random.RandomState(seed)
    ids = np.arange(n_points, dtype=np.int64)
    pts = rng.uniform(-0.6, 0.6, (n_points, 2))
    next_id = n_points
    out = []
    steps = [0.05, 0.004, 0.06, 0.05, 0.003, 0.04, 0.005, 0.05, 0.002, 0.06, 0.004, 0.05, 0.003, 0.04, 0.05, 0.004]
    for f in range(n_frames):
        fc = min(f, fu.WINDOW_SIZE)
        order = rng.permutation(n_points)
        big = ids * ID_SCALE + ID_SHIFT if big_ids else ids
        out.append((fc, big[order].copy(), pts[order].copy()))
        keep = rng.uniform(size=n_points) < survive
        d = rng.normal(size=(n_points, 2))
        pts = pts + steps[f % len(steps)] * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n_points, 1))
        lost = np.nonzero(~keep)[0]
        ids[lost] = np.arange(next_id, next_id + len(lost))
        pts[lost] = rng.uniform(-0.6, 0.6, (len(lost), 2))
        next_id += len(lost)
    return out


def main():
    ref = fu.RefFeatureManager(C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libvio_ref.so")))
    frames = make_frames(2026)
    tracks, keys, lasts = [], [], []
    for fc, ids, pts in frames:
        small = (ids - ID_SHIFT) // ID_SCALE
        assert np.array_equal(small * ID_SCALE + ID_SHIFT, ids) and small.max() < 2 ** 31
        key, last = ref.add_image(fc, small, pts)
        tracks, res = fr.add(tracks, fc, ids, pts)
        assert (res["keyframe"], res["last_track_num"]) == (int(key), last), (fc, res, key, last)
        if res["parallax_num"]:
            mean = res["parallax_sum_ref"] / res["parallax_num"]
            assert abs(mean - fr.MIN_PARALLAX) >= 1e-6 * fr.MIN_PARALLAX, (fc, mean)
        keys.append(int(key))
        lasts.append(last)
        if fc == fu.WINDOW_SIZE:
            op = (5,) if key else (6, fu.WINDOW_SIZE)
            ref.apply(op)
            tracks = fr.apply_op(tracks, op)
    assert 0 < sum(keys) < len(keys), keys
    want = ref.tracks()
    for t in want:
        t["id"] = t["id"] * ID_SCALE + ID_SHIFT
    fr.assert_tracks_equal(tracks, fr.copy_tracks(want))          # the restatement agrees before anything is written
    ids, start, depth, flag, off, pts = fr.tracks_to_arrays(fr.copy_tracks(want))
    path = os.path.join(HERE, "fm_large.npz")
    np.savez_compressed(path, seq_ids=np.concatenate([f[1] for f in frames]), seq_pts=np.concatenate([f[2] for f in frames]),
                        seq_off=np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])]).astype(np.int64),
                        seq_frame_count=np.array([f[0] for f in frames], dtype=np.int32), seq_key=np.array(keys, dtype=np.int32),
                        seq_last_track_num=np.array(lasts, dtype=np.int32), seq_out_id=ids, seq_out_start=start, seq_out_depth=depth,
                        seq_out_flag=flag, seq_out_off=off, seq_out_pts=pts)
    print("%s: %d bytes, %d final tracks, keys %s" % (path, os.path.getsize(path), len(want), keys))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
