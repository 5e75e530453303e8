"""tests/fm_reference.py (what libvio_fm_hip is held to, include/vio_fm.h) against the compiled reference's recorded outputs:
tests/golden/feature_manager.npz (the parallax sequence and the six scenarios) and tests/golden/fm_large.npz (a sequence of about 600
points per frame, tests/golden/make_golden_fm.py), and, where the compiled reference is, against it live on fresh seeds."""
import os

import numpy as np
import pytest

import fm_reference as fr
import fm_util as fu
from conftest import GOLDEN_DIR, ORACLE_DIR

TRI_RTOL = 1e-7                                          # tests/test_feature_manager_golden.py's figure for the same data


@pytest.fixture(scope="module")
def fmz():
    return np.load(os.path.join(GOLDEN_DIR, "feature_manager.npz"))


def replay_sequence(z, p="par_"):
    """The frames of a recorded sequence through the restatement; the decisions, last_track_num and the final tracks."""
    tracks, keys, lasts, margins = [], [], [], []
    for f in range(len(z[p + "frame_count"])):
        lo, hi = z[p + "off"][f], z[p + "off"][f + 1]
        fc = int(z[p + "frame_count"][f])
        tracks, res = fr.add(tracks, fc, z[p + "ids"][lo:hi], z[p + "pts"][lo:hi])
        assert res["status"] == fr.STATUS_OK
        keys.append(res["keyframe"])
        lasts.append(res["last_track_num"])
        if res["parallax_num"]:
            mean = res["parallax_sum_ref"] / res["parallax_num"]
            margins.append(abs(mean - fr.MIN_PARALLAX) / fr.MIN_PARALLAX)
            # the two orders: at most 2 (n - 1) 2^-53 of the sum apart
            assert abs(res["parallax_sum"] - res["parallax_sum_ref"]) <= 2 * (res["parallax_num"] - 1) * 2.0 ** -53 * res["parallax_sum_ref"]
        if fc == fu.WINDOW_SIZE:                         # Estimator::slideWindow, as the generator did
            tracks = fr.slide(tracks, fr.BACK) if res["keyframe"] else fr.slide(tracks, fr.FRONT, fu.WINDOW_SIZE)
    return tracks, keys, lasts, margins


def test_parallax_sequence_matches_the_golden(fmz):
    tracks, keys, lasts, margins = replay_sequence(fmz)
    np.testing.assert_array_equal(keys, fmz["par_key"])
    np.testing.assert_array_equal(lasts, fmz["par_last_track_num"])
    assert 0 < sum(keys) < len(keys)
    assert min(margins) >= 0.75                          # (0.7595 here) no decision of the sequence hinges on the order of the sum
    fr.assert_tracks_equal(tracks, fr.copy_tracks(fu.arrays_to_tracks(fmz, "par_out_")))


def test_large_sequence_matches_the_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "fm_large.npz"))
    tracks, keys, lasts, margins = replay_sequence(z, "seq_")
    np.testing.assert_array_equal(keys, z["seq_key"])
    np.testing.assert_array_equal(lasts, z["seq_last_track_num"])
    assert 0 < sum(keys) < len(keys) and min(margins) >= 1e-6
    assert z["seq_ids"].max() > 2 ** 31 and len(tracks) > 160
    want = fr.arrays_to_tracks(dict(ids=z["seq_out_id"], start=z["seq_out_start"], depth=z["seq_out_depth"], flag=z["seq_out_flag"],
                                    off=z["seq_out_off"], pts=z["seq_out_pts"]))
    fr.assert_tracks_equal(tracks, want)


@pytest.mark.parametrize("name", fu.SCENARIOS)
def test_scenarios_match_the_golden(fmz, name):
    p = "sc_%s_" % name
    tracks = fr.copy_tracks(fu.arrays_to_tracks(fmz, p + "in_"))
    ops = fu.arrays_to_ops(fmz, p + "op_")
    for op in ops:
        tracks = fr.apply_op(tracks, op, fmz[p + "poses"], fmz[p + "ext"])
    want = fu.arrays_to_tracks(fmz, p + "out_")
    has_tri = any(op[0] == 1 for op in ops)
    fu.compare_tracks(tracks, want, depth_rtol=TRI_RTOL if has_tri else 1e-14)      # (ids, starts, flags and points byte-equal in there)
    assert fr.counts(tracks)[1] == int(fmz[p + "count"])
    np.testing.assert_allclose(fr.export(tracks)["inv_depth"], fmz[p + "depvec"], rtol=TRI_RTOL if has_tri else 1e-14)
    if any(op[0] == 4 for op in ops) and not has_tri:   # the depth shift against the reference, inside its forward error bound
        src = {t["id"]: t for t in fu.arrays_to_tracks(fmz, p + "in_")}
        op = [o for o in ops if o[0] == 4][0]
        n = 0
        for g, w in zip(tracks, want):
            s = src[g["id"]]
            if s["start"] == 0 and w["depth"] != fr.INIT_DEPTH:
                assert abs(g["depth"] - w["depth"]) <= fr.shift_depth_bound(s["pts"][0][0], s["pts"][0][1], s["depth"], *op[1:5])
                n += 1
        assert n > 0 or name == "behind_camera"


def test_slide_row_covers_every_branch():
    seen = set()
    for kind in (fr.BACK_SHIFT_DEPTH, fr.BACK, fr.FRONT):
        for fc in range(1, 11):
            for start in range(0, 11):
                for k in range(1, 12 - start):
                    s = fr.slide_row(kind, fc, start, k)
                    assert s[1] < k and (s[1] < 0 or k - 1 >= 0)
                    seen.add((kind, s[1] >= 0, s[2], s[3], s[0] != start))
    assert len(seen) >= 9


@pytest.mark.ref
@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_matches_the_compiled_reference_on_fresh_seeds(seed):
    """About 600 points per frame through add and the slides, then set_depth, removeFailures and a depth shift: the restatement against
    the reference's FeatureManager itself."""
    import ctypes as C
    so = os.path.join(ORACLE_DIR, "_ref", "libvio_ref.so")
    if not os.path.exists(so):
        pytest.skip("oracle/_ref is only buildable where the reference is")
    import sys
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_fm as mg
    ref = fu.RefFeatureManager(C.CDLL(so))
    frames = mg.make_frames(seed + 100, n_frames=13, n_points=600, big_ids=False)
    tracks = []
    for fc, ids, pts in frames:
        key, last = ref.add_image(fc, ids, pts)
        tracks, res = fr.add(tracks, fc, ids, pts)
        assert (res["keyframe"], res["last_track_num"]) == (int(key), last)
        if fc == fu.WINDOW_SIZE:
            op = (5,) if key else (6, fu.WINDOW_SIZE)
            ref.apply(op)
            tracks = fr.apply_op(tracks, op)
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.05, 0.5, fr.counts(tracks)[1])
    x[::9] *= -1.0
    R0, R1 = mg.random_rotation(rng), mg.random_rotation(rng)
    for op in [(2, x), (3,), (4, R0, rng.uniform(-1, 1, 3), R1, rng.uniform(-1, 1, 3))]:
        ref.apply(op)
        tracks = fr.apply_op(tracks, op)
    fu.compare_tracks(tracks, ref.tracks(), depth_rtol=1e-12)
    assert len(tracks) > 1000
