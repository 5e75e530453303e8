"""tests/fm_outlier_reference.py's remove_ids against what the compiled reference's FeatureManager recorded: with the ids of the
solve_flag == 2 rows it is removeFailures (feature_manager.cpp:161-171), the loop removeOutlier (:259-275) has behind its `return;`.
tests/golden/feature_manager.npz's scenarios `depth_vector` and `frame_chain` hold the reference's own lists after setDepth and
removeFailures; tests/golden/fm_large.npz a list of a few hundred tracks with ids above 2^31."""
import os

import numpy as np
import pytest

import fm_outlier_reference as fo
import fm_reference as fr
import fm_util as fu
from conftest import GOLDEN_DIR

TRI_RTOL = 1e-7                                          # tests/test_fm_reference.py's figure for the scenarios that triangulate


@pytest.fixture(scope="module")
def fmz():
    return np.load(os.path.join(GOLDEN_DIR, "feature_manager.npz"))


def failed_ids(tracks):
    return np.array([t["id"] for t in tracks if t["flag"] == 2], dtype=np.int64)


def test_depth_vector_scenario_by_id_is_the_references_remove_failures(fmz):
    p = "sc_depth_vector_"
    ops = fu.arrays_to_ops(fmz, p + "op_")
    assert [op[0] for op in ops] == [2, 3]
    tracks = fr.set_depth(fr.copy_tracks(fu.arrays_to_tracks(fmz, p + "in_")), ops[0][1])
    ids = failed_ids(tracks)
    assert 0 < len(ids) < len(tracks)
    got, erased = fo.remove_ids(tracks, ids)
    assert erased.all() and len(got) == len(tracks) - len(ids)
    fu.compare_tracks(got, fu.arrays_to_tracks(fmz, p + "out_"), depth_rtol=1e-14)       # (ids, starts, flags, points byte-equal in there)
    assert fr.counts(got)[1] == int(fmz[p + "count"])


def test_frame_chain_scenario_with_the_erase_by_id(fmz):
    p = "sc_frame_chain_"
    ops = fu.arrays_to_ops(fmz, p + "op_")
    assert [op[0] for op in ops[:3]] == [1, 2, 3]
    tracks = fr.copy_tracks(fu.arrays_to_tracks(fmz, p + "in_"))
    for op in ops[:2]:
        tracks = fr.apply_op(tracks, op, fmz[p + "poses"], fmz[p + "ext"])
    ids = failed_ids(tracks)
    assert len(ids) > 0
    by_id, erased = fo.remove_ids(tracks, ids[::-1])                                  # (the order of the ids does not matter)
    assert erased.all()
    fr.assert_tracks_equal(by_id, fr.remove_failures(tracks))
    tracks = by_id
    for op in ops[3:]:
        tracks = fr.apply_op(tracks, op, fmz[p + "poses"], fmz[p + "ext"])
    fu.compare_tracks(tracks, fu.arrays_to_tracks(fmz, p + "out_"), depth_rtol=TRI_RTOL)


def large_tracks():
    z = np.load(os.path.join(GOLDEN_DIR, "fm_large.npz"))
    return fr.arrays_to_tracks(dict(ids=z["seq_out_id"], start=z["seq_out_start"], depth=z["seq_out_depth"], flag=z["seq_out_flag"],
                                    off=z["seq_out_off"], pts=z["seq_out_pts"]))


def test_large_list_by_id_is_remove_failures():
    tracks = large_tracks()
    x = np.linspace(0.1, 0.5, fr.counts(tracks)[1])
    x[::9] *= -1.0
    tracks = fr.set_depth(tracks, x)
    ids = failed_ids(tracks)
    assert len(ids) >= 10 and max(t["id"] for t in tracks) > 2 ** 31
    got, erased = fo.remove_ids(tracks, ids)
    assert erased.all()
    fr.assert_tracks_equal(got, fr.remove_failures(tracks))


def test_absent_empty_all_and_extreme_ids():
    tracks = large_tracks()
    have = np.array([t["id"] for t in tracks], dtype=np.int64)
    got, erased = fo.remove_ids(tracks, [])
    assert erased.shape == (0,)
    fr.assert_tracks_equal(got, fr.copy_tracks(tracks))
    absent = np.array([-1, -2 ** 63, 2 ** 63 - 1, 2 ** 31 + 5, 2 ** 40 + 1], dtype=np.int64)
    absent = absent[~np.isin(absent, have)]
    assert len(absent) >= 3
    got, erased = fo.remove_ids(tracks, absent)
    assert not erased.any()
    fr.assert_tracks_equal(got, fr.copy_tracks(tracks))
    got, erased = fo.remove_ids(tracks, have[::-1])
    assert got == [] and erased.all()
    # ids above 2^31 and negative that are there
    odd = fr.copy_tracks(tracks[:6])
    for t, i in zip(odd, (-7, 2 ** 31 + 1, -2 ** 63, 2 ** 63 - 1, 3, 2 ** 52 + 1)):
        t["id"] = i
    mixed = np.array([2 ** 63 - 1, 11, -7, 2 ** 31 + 1], dtype=np.int64)
    got, erased = fo.remove_ids(odd, mixed)
    assert list(erased) == [True, False, True, True] and [t["id"] for t in got] == [-2 ** 63, 3, 2 ** 52 + 1]
    fr.assert_tracks_equal(got, [odd[2], odd[4], odd[5]])
    with pytest.raises(ValueError):
        fo.remove_ids(odd, [3, 3])
