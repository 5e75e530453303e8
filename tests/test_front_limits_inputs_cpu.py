"""The inputs of tests/test_gpu_front_limits.py's full-table scenario (tests/front_limits_inputs.py) through the numpy restatements of
the three stages: flow_reference.multi_level (order "wave64"), reject_reference.reject and detect_reference.detect, with equalize off,
the forward flow, 2 levels, half_patch 2, border 1 and min_distance 2.  What the GPU scenario asserts of its oracle's arrays holds
here on the restatement alone, so the inputs are known to reach past a wavefront and a workgroup before a GPU sees them.

Frame 0 into frame 1, as observed (COUNTS below holds what is asserted):
    detection on frame 0    1024 of 1413 candidates
    filter                  989 of 1024 rows kept, rows dropped in 14 of the 16 wavefronts
    rejectWithF (pair 1)    917 of 989 rows kept, rows dropped in 15 of the 16 wavefronts of its input, status OK, margin 2.6e-3
    setMask                 853 of 917 rows kept; 171 new points: 1024 rows again
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as flow_ref  # noqa: E402
import front_limits_inputs as fl  # noqa: E402
import reject_reference as rr  # noqa: E402


@pytest.fixture(scope="module")
def stages():
    """Every stage of frame 0 and of frame 1, once."""
    a, b = np.ascontiguousarray(fl.image(0)), np.ascontiguousarray(fl.image(1))
    first = dr.detect(a, max_total=fl.CAP, min_distance=fl.MIN_DIST)
    cur = first["new_pts"].astype(np.float32)
    forw, status, _, _ = flow_ref.multi_level(a, b, cur, None, inverse=0, border=fl.BORDER, order="wave64", **fl.FLOW)
    r = np.rint(forw.astype(np.float64))
    with np.errstate(invalid="ignore"):
        inside = (fl.BORDER <= r[:, 0]) & (r[:, 0] < fl.W - fl.BORDER) & (fl.BORDER <= r[:, 1]) & (r[:, 1] < fl.H - fl.BORDER)
    keep = (status == 0) & inside
    rej = rr.reject(rr.Camera(**fl.CAM), cur[keep], forw[keep], 1, fl.RANSAC)
    tracked = forw[keep][rej["mask"]]
    det = dr.detect(b, tracked, np.full(len(tracked), 2, np.int32), None, fl.CAP, min_distance=fl.MIN_DIST)
    print("frame 0: %d of %d candidates; filter %d of %d, drops in wavefronts %s; reject %d of %d, status %d, margin %.2g, drops in "
          "wavefronts %s; setMask %d of %d, %d new" % (first["n_new"], first["n_candidates"], keep.sum(), len(keep), fl.waves_with_drops(keep),
                                                       rej["mask"].sum(), len(rej["mask"]), rej["status"], rej["margin"],
                                                       fl.waves_with_drops(rej["mask"]), det["n_kept"], len(tracked), det["n_new"]))
    return dict(first=first, keep=keep, rej=rej, tracked=tracked, det=det)


def test_the_stream_is_what_the_gpu_tests_expect():
    a, b = fl.image(0), fl.image(1)
    assert a.shape == b.shape == (fl.H, fl.W) and a.dtype == np.uint8
    assert np.array_equal(a, fl.fs.image(fl.W, fl.H, fl.SEED, 0))                   # frame 0 is the plain stream
    plain = fl.fs.image(fl.W, fl.H, fl.SEED, 1)
    assert np.array_equal(b[~fl.planted()], plain[~fl.planted()]) and np.mean(b[fl.planted()] != plain[fl.planted()]) > 0.5
    assert 0.2 < fl.planted().mean() < 0.3
    assert fl.image(2).strides[0] != fl.W                                           # every third frame has strided rows
    pts, ids, cnt = fl.seeded(fl.CAP)
    assert len(pts) == fl.CAP and len(set(ids.tolist())) == fl.CAP and set(cnt.tolist()) == {2, 3, 4, 5, 6}
    assert len(set(map(tuple, np.rint(pts).astype(int).tolist()))) == fl.CAP        # distinct pixels
    s = fl.strong(fl.CAP)                                                           # enough strong rows for the whole-wavefront scenario
    assert len(s) == fl.CAP and np.all(fl.inner(s, 11)) and not np.all(fl.inner(pts, 11))
    m = fl.margin_points(960)
    assert np.all(m[:, 0] == 3.0) and m[:, 1].min() >= 10 and m[:, 1].max() < fl.H - 10


def test_frame_0_fills_the_table(stages):
    assert stages["first"]["n_new"] == fl.CAP and stages["first"]["n_candidates"] > fl.CAP


def test_the_filter_drops_rows_in_many_wavefronts(stages):
    keep = stages["keep"]
    assert len(keep) == fl.CAP and keep.sum() > 512 and len(fl.waves_with_drops(keep)) >= 4


def test_reject_keeps_most_and_drops_in_many_wavefronts(stages):
    rej = stages["rej"]
    assert len(rej["mask"]) >= 8 and rej["status"] == rr.OK and rej["hyp"] >= 0
    assert rej["mask"].sum() > 512 and len(fl.waves_with_drops(rej["mask"])) >= 4
    assert rej["margin"] > 1e-6                                                     # no error at the gate: the mask is well defined


def test_set_mask_strikes_and_the_table_fills_again(stages):
    det, n = stages["det"], len(stages["tracked"])
    assert 0 < det["n_kept"] < n and not np.array_equal(det["keep_order"], np.arange(det["n_kept"]))
    assert det["n_new"] > 0 and det["n_kept"] + det["n_new"] == fl.CAP
