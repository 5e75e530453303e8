"""The forward-backward check of the batched Lucas-Kanade tracker (k_flow_track<INV, true>, include/vio_flow_back.h)
where kernels go wrong: patches that leave lanes idle, give a lane a ragged second term, 7 or 16 terms; a backward pyramid shorter than
the forward one, as tall as it, or of one level; a forward pass that has a guess itself; max_iter 1 and early_stop on; point counts
around the four keypoints of a workgroup and the 64 rows of a wavefront, up to 1024 rows; items that start at flow offsets that are no
multiple of 4; strided rows; items of different sizes in one call; max_dist one double below, at and above sqrt(d2); the resident twin.

The inputs and their numpy restatements are tests/flow_back_limits_inputs.py's, which tests/test_flow_back_limits_inputs_cpu.py holds to
what is assumed here.  The comparison is tests/test_gpu_flow_back.py's against_restatement: next_pts, both statuses, back_pts, both
iteration counts and d2 byte for byte, the two costs under that file's rule (the NaNs in the same places, rtol = atol = 1e-9).  Every
case prints its outcome counts and asserts from the restatement that it reached the backward pass.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_limits_inputs as bl  # noqa: E402
import flow_back_reference as fb  # noqa: E402
from test_gpu_flow_back import ALL, against_restatement, bytes_of, same  # noqa: E402

pytestmark = pytest.mark.gpu
FORWARD = ("next_pts", "status", "iterations", "cost")
MIN_BACK_PASSES, MIN_SMALL_BACK_PASSES = 40, 54     # tests/test_flow_back_limits_inputs_cpu.py's


@pytest.fixture(scope="module")
def flow_lib(vio, hip_lib):
    return vio.load_flow()


@pytest.fixture()
def fh(flow_lib):
    h = flow_lib.create()
    yield h
    h.close()


def run_case(fh, case, a, b, pts, guess, min_passes):
    ref = bl.restate(case)
    c = fb.counts(ref)
    assert c["forward_ok"] >= min_passes, c
    fh.set_config(levels=case["levels"], inverse=case["inverse"], **case["flow"])
    fh.set_back(levels=case["back_levels"])
    got = fh.track(a, b, pts, guess, back=True)
    against_restatement(got, ref, case["name"])
    plain = fh.track(a, b, pts, guess)                                  # the verdict without the rows
    assert sorted(plain) == sorted(FORWARD)
    same(plain, got, case["name"] + ": track without the rows", FORWARD)
    return ref


@pytest.mark.parametrize("case", bl.settings(), ids=lambda c: c["name"])
def test_settings(fh, case):
    a, b, pts, g = bl.settings_inputs(case)
    ref = run_case(fh, case, a, b, pts, g, MIN_BACK_PASSES)
    n, c = len(pts), fb.counts(ref)
    assert 0.1 * n < c["kept"] < 0.9 * n, c


@pytest.mark.parametrize("case", bl.small(), ids=lambda c: c["name"])
def test_small(fh, case):
    a, b, pts = bl.small_inputs()
    run_case(fh, case, a, b, pts, None, MIN_SMALL_BACK_PASSES)


def full_handle(fh, inverse, back_levels=bl.FULL_CFG["back_levels"]):
    cfg = {k: v for k, v in bl.FULL_CFG.items() if k != "back_levels"}
    fh.set_config(inverse=inverse, **cfg)
    fh.set_back(levels=back_levels)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257, 1024])
def test_point_counts(fh, n, inverse):
    a, b, pts = bl.full_inputs()
    ref = bl.prefix(bl.full(inverse), n)
    assert np.any(ref["back_status"] != fb.BACK_NOT_RUN)
    full_handle(fh, inverse)
    got = fh.track(a, b, pts[:n], back=True)
    against_restatement(got, ref, "the first %d rows, inv%d" % (n, inverse))
    if n == bl.CAP:
        c = fb.counts(ref)
        assert min(c["forward_lost"], c["back_lost"], c["back_far"]) >= 3 and len(bl.failed_groups(ref)) >= 12, c


@pytest.mark.parametrize("inverse", [0, 1])
def test_four_items_at_odd_flow_offsets(fh, inverse):
    """5, 0, 63 and 130 rows of one pair: the later items start at rows 5, 5 and 68 of the call's flat keypoint list."""
    a, b, pts = bl.full_inputs()
    full = bl.full(inverse)
    cuts = [(0, 5), (5, 5), (5, 68), (68, 198)]
    items = [dict(img_prev=a, img_next=b, prev_pts=pts[lo:hi]) for lo, hi in cuts]
    full_handle(fh, inverse)
    outs = fh.track_batch(items, back=True)
    assert [len(o["status"]) for o in outs] == [5, 0, 63, 130]
    for (lo, hi), it, o in zip(cuts, items, outs):
        ref = bl.prefix(full, hi, lo)
        assert hi == lo or np.sum(ref["back_status"] != fb.BACK_NOT_RUN) >= 3
        against_restatement(o, ref, "rows %d .. %d, inv%d" % (lo, hi, inverse))
        assert bytes_of(fh.track_batch([it], back=True)[0]) == bytes_of(o), (lo, hi)
    again = fh.track_batch(items, back=True)
    assert [bytes_of(o) for o in again] == [bytes_of(o) for o in outs]


@pytest.mark.parametrize("inverse", [0, 1])
def test_strided_rows(fh, inverse):
    a, b, pts = bl.strided()
    assert a.strides[0] == b.strides[0] == a.shape[1] + bl.PAD
    ref = fb.fixture_reference(inverse, 2)
    assert fb.counts(ref)["forward_ok"] >= MIN_BACK_PASSES
    fh.set_config(levels=fb.FIXTURE_LEVELS, inverse=inverse)
    fh.set_back(levels=2)
    against_restatement(fh.track(a, b, pts, back=True), ref, "strided rows, inv%d" % inverse)


@pytest.mark.parametrize("back_levels,inverse", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_items_of_different_sizes(fh, back_levels, inverse):
    """192 x 144, 96 x 72 and 33 x 25 in one call: each item's level sizes and pitches are its own, in both passes."""
    items = [dict(img_prev=a, img_next=b, prev_pts=p) for a, b, p in bl.mixed_items()]
    refs = bl.mixed(back_levels, inverse)
    fh.set_config(inverse=inverse, **bl.MIXED_CFG)
    fh.set_back(levels=back_levels)
    outs = fh.track_batch(items, back=True)
    for i, (it, o, ref) in enumerate(zip(items, outs, refs)):
        assert fb.counts(ref)["forward_ok"] >= MIN_BACK_PASSES
        against_restatement(o, ref, "item %d of three, back levels %d, inv%d" % (i, back_levels, inverse))
        assert bytes_of(fh.track_batch([it], back=True)[0]) == bytes_of(o), i


@pytest.mark.parametrize("inverse", [0, 1])
def test_max_dist_next_to_sqrt_d2(fh, inverse):
    """max_dist one double below, at and above sqrt(d2) of three rows: the verdict is d2 <= max_dist * max_dist in doubles, for the row
    and for every other row; nothing else of the call moves."""
    a, b, pts = fb.fixture()
    ref = fb.fixture_reference(inverse, 2)
    picked = bl.boundary_pick(ref, 3)
    assert len(picked) == 3 and bl.has_exact(ref["back_d2"][picked[0][0]], picked[0][1])
    fh.set_config(levels=fb.FIXTURE_LEVELS, inverse=inverse)
    fh.set_back(levels=2)
    base = fh.track(a, b, pts, back=True)
    against_restatement(base, ref, "the base call, inv%d" % inverse)
    came_back = ref["back_status"] == fb.OK
    for r, ms in picked:
        seen = set()
        for m in ms:
            fh.set_back(levels=2, max_dist=m)
            got = fh.track(a, b, pts, back=True)
            want = bl.verdict_at(ref["back_d2"][r], m)
            seen.add(want)
            print("inv%d row %d d2 %.17g max_dist %.17g: %d (expected %d)" % (inverse, r, ref["back_d2"][r], m, got["status"][r], want))
            assert got["status"][r] == want, (r, m)
            same(got, base, "max_dist %.17g" % m, tuple(k for k in ALL if k != "status"))
            expect = ref["status"].copy()
            expect[came_back] = [bl.verdict_at(d, m) for d in ref["back_d2"][came_back]]
            assert np.array_equal(got["status"], expect), (r, m)
        assert seen == {fb.OK, fb.FAIL_BACK_FAR}, r


@pytest.mark.parametrize("inverse", [0, 1])
def test_resident_twin_at_a_full_table(vio, hip_lib, fh, inverse):
    """vio_frame_track_back_batch on the 192 x 144 pair in a slot, 1024 rows and 65: the host-array call's bytes, and the restatement's."""
    a, b, pts = bl.full_inputs()
    cfg = {k: v for k, v in bl.FULL_CFG.items() if k != "back_levels"}
    full_handle(fh, inverse)
    fr_h = vio.load_frame().create()
    try:
        fr_h.set_config(equalize=False, flow=dict(inverse=inverse, **cfg))
        fr_h.set_flow_back(levels=bl.FULL_CFG["back_levels"])
        fr_h.push(a, slot=5)
        fr_h.push(b, slot=5)
        for n in (bl.CAP, 65):
            got, host = fr_h.track(pts[:n], slot=5, back=True), fh.track(a, b, pts[:n], back=True)
            same(got, host, "resident, %d rows, inv%d" % (n, inverse))
            against_restatement(got, bl.prefix(bl.full(inverse), n), "resident, %d rows, inv%d" % (n, inverse))
        # a resident frame 33 pixels wide has rows 36 bytes apart: the one place where a level's pitch is not its width on the device
        sa, sb, sp = bl.small_inputs()
        fr_h.push(sa, slot=6)
        fr_h.push(sb, slot=6)
        ref = bl.mixed(bl.FULL_CFG["back_levels"], inverse)[2]
        assert fb.counts(ref)["forward_ok"] >= MIN_BACK_PASSES
        both = fr_h.track_batch([dict(slot=5, prev_pts=pts[:65]), dict(slot=6, prev_pts=sp)], back=True)
        against_restatement(both[1], ref, "resident, 33 x 25, inv%d" % inverse)
        same(both[1], fh.track(sa, sb, sp, back=True), "resident, 33 x 25, inv%d" % inverse)
        same(both[0], got, "resident, 65 rows beside the 33 x 25 slot")
    finally:
        fr_h.close()
