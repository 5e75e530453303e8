"""tests/flow_back_limits_inputs.py held to what tests/test_gpu_flow_back_limits.py and tests/test_gpu_front_back_limits.py assume of it,
on the numpy restatement alone (tests/flow_back_reference.track_back), so that a GPU test never passes by meeting nothing.

As computed on a CPU (OK forwards / lost forwards / lost backwards / far / kept):
    full(0)    989 / 35 / 9 / 40 / 940, a failed check in every one of the sixteen 64-row groups
    full(1)    993 / 31 / 3 / 54 / 936
    settings() SETTINGS_COUNTS of the inputs module, asserted exactly; every case keeps between 10 % and 90 % of its rows and runs at
               least 40 backward passes
    small()    54 to 108 backward passes in each case
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_limits_inputs as bl  # noqa: E402
import flow_back_reference as fb  # noqa: E402

ARRAYS = ("next_pts", "status", "iterations", "cost", "back_pts", "back_status", "back_iterations", "back_cost", "back_d2")
MIN_OUTCOMES = {0: 5, 1: 3}                          # rows of each outcome on full(inverse)
MIN_FAILED_GROUPS = 12
MIN_BACK_PASSES, MIN_SMALL_BACK_PASSES = 40, 54


def same(x, y, name):
    for k in ARRAYS:
        assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), (name, k)


@pytest.mark.parametrize("inverse", [0, 1])
def test_full_reaches_every_outcome(inverse):
    ref = bl.full(inverse)
    c = fb.counts(ref)
    print("full(%d): %s, failed checks in groups %s" % (inverse, c, bl.failed_groups(ref)))
    assert len(ref["status"]) == bl.CAP
    assert min(c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) >= MIN_OUTCOMES[inverse], c
    assert c["forward_ok"] == c["kept"] + c["back_lost"] + c["back_far"] and c["kept"] > bl.CAP // 2
    assert bl.back_info(ref) == dict(n_checked=c["forward_ok"], n_back_lost=c["back_lost"], n_back_far=c["back_far"])
    if inverse == 0:
        assert len(bl.failed_groups(ref)) >= MIN_FAILED_GROUPS
        assert (c["forward_ok"], c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) == (989, 35, 9, 40, 940), c
    else:
        assert (c["forward_ok"], c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) == (993, 31, 3, 54, 936), c
    # the prefixes the GPU tests cut reach the backward pass, and the four-item call's slices do too
    for n in (3, 4, 5):
        assert np.any(ref["back_status"][:n] != fb.BACK_NOT_RUN), n
    for lo, hi in ((0, 5), (5, 68), (68, 198)):
        assert np.sum(ref["back_status"][lo:hi] != fb.BACK_NOT_RUN) >= 3, (lo, hi)


@pytest.mark.parametrize("inverse", [0, 1])
def test_a_prefix_of_the_rows_is_a_prefix_of_the_restatement(inverse):
    a, b, pts = bl.full_inputs()
    same(fb.track_back(a, b, pts[:65], inverse=inverse, **bl.FULL_CFG), bl.prefix(bl.full(inverse), 65), "the first 65 rows")


@pytest.mark.parametrize("case", bl.settings(), ids=lambda c: c["name"])
def test_settings_reach_the_backward_pass(case):
    ref = bl.restate(case)
    c = fb.counts(ref)
    print(case["name"], c)
    n = len(ref["status"])
    assert n == 140 and 0.1 * n < c["kept"] < 0.9 * n and c["forward_ok"] >= MIN_BACK_PASSES, c
    if case["name"] in bl.SETTINGS_COUNTS:
        assert (c["forward_ok"], c["kept"], c["back_lost"], c["back_far"]) == bl.SETTINGS_COUNTS[case["name"]], c
    if case["flow"].get("max_iter") == 1:
        assert set(ref["iterations"].tolist()) == {1} and set(ref["back_iterations"][ref["back_status"] != fb.BACK_NOT_RUN].tolist()) == {1}


def test_the_early_stop_cases_differ():
    off, on = (bl.restate(c) for c in bl.settings() if c["name"].startswith("early_stop"))
    same(off, fb.fixture_reference(0, 2), "early_stop 0 is the default")
    assert off["status"].tobytes() != on["status"].tobytes() and off["back_iterations"].tobytes() != on["back_iterations"].tobytes()


@pytest.mark.parametrize("case", bl.small(), ids=lambda c: c["name"])
def test_small_reaches_the_backward_pass(case):
    ref = bl.restate(case)
    c = fb.counts(ref)
    print(case["name"], c)
    assert len(ref["status"]) == 108 and c["forward_ok"] >= MIN_SMALL_BACK_PASSES, c
    if case["flow"]["half_patch"] > 2:
        assert c["forward_lost"] >= 10, c                               # the grid's outer points: their patch leaves the image


def test_strided_is_the_contiguous_pair():
    a, b, pts = bl.strided()
    ca, cb, cpts = fb.fixture()
    assert a.strides == b.strides == (96 + bl.PAD, 1) and not a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, ca) and np.array_equal(b, cb) and np.array_equal(pts, cpts)
    assert np.all(a.base[:, 96:] == 255) and np.all(b.base[:, 96:] == 255)
    same(fb.track_back(a, b, pts, levels=fb.FIXTURE_LEVELS, back_levels=2), fb.fixture_reference(0, 2), "strided")


@pytest.mark.parametrize("back_levels,inverse", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_mixed_items_reach_the_backward_pass(back_levels, inverse):
    refs = bl.mixed(back_levels, inverse)
    assert [len(r["status"]) for r in refs] == [bl.MIXED_ROWS, 140, 108]
    for r in refs:
        c = fb.counts(r)
        print(back_levels, inverse, c)
        assert c["forward_ok"] >= MIN_BACK_PASSES and c["kept"] >= 5 and c["back_lost"] + c["back_far"] >= 1, c


@pytest.mark.parametrize("inverse", [0, 1])
def test_boundary_rows_give_both_verdicts(inverse):
    ref = fb.fixture_reference(inverse, 2)
    rows = bl.boundary_rows(ref)
    picked = bl.boundary_pick(ref, 3)
    print("inverse %d: %d boundary rows, picked %s" % (inverse, len(rows), [(r, float(ref["back_d2"][r])) for r, _ in picked]))
    assert len(rows) >= 3 and len(picked) == 3
    for r, (lo, mid, hi) in picked:
        d2 = ref["back_d2"][r]
        assert lo < mid < hi and mid * mid <= np.nextafter(d2, np.inf) and ref["back_status"][r] == fb.OK
        assert bl.verdict_at(d2, lo) == fb.FAIL_BACK_FAR and bl.verdict_at(d2, hi) == fb.OK
        # flow_back_reference.verdict is the same rule
        for m in (lo, mid, hi):
            assert fb.verdict(True, fb.fixture()[2][r], ref["back_pts"][r], m) == (bl.verdict_at(d2, m), float(d2))
    # a row whose d2 is the exact square of one of its three values: there `<` for `<=` gives another verdict
    r, ms = picked[0]
    assert bl.has_exact(ref["back_d2"][r], ms)
