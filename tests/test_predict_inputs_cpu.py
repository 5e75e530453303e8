"""What tests/test_gpu_fm_predict.py assumes of tests/predict_inputs.py's tables, asserted without a device: every mixed case has rows
on both sides of each of the three conditions of the rule, the full table predicts at least half of its rows and not all, one 64-row
group (the rows of one ballot) predicts all of its rows and one predicts none, and the tables are ones vio_fm_tracks_set accepts."""
import numpy as np
import pytest

import fm_predict_reference as fp
import predict_inputs as pi


def conditions(t, fc):
    nobs = t["off"][1:] - t["off"][:-1]
    return t["depth"] > 0, nobs >= 2, t["start"] + nobs - 1 == fc


@pytest.mark.parametrize("n,fc", pi.MIXED)
def test_rows_on_both_sides_of_every_condition(n, fc):
    t, kinds = pi.table(n, fc)
    cond = conditions(t, fc)
    for c in cond:
        assert c.any() and (~c).any()
    # ... and each condition decides alone somewhere: a row that fails only it
    for i in range(3):
        others = np.logical_and.reduce([c for j, c in enumerate(cond) if j != i])
        assert (others & ~cond[i]).any()
    q = fp.qualifies(t["start"], t["off"][1:] - t["off"][:-1], t["depth"], fc)
    assert np.array_equal(q, kinds == pi.QUALIFIES) and 0 < q.sum() < n
    assert np.any(t["depth"][q] < 2.3e-308) or n < 1000       # denormal depths among the rows that qualify


def test_tables_are_ones_tracks_set_accepts():
    for n, fc in list(pi.MIXED) + [(1, 10), (0, 10), (65, 1)]:
        t, _ = pi.table(n, fc)
        nobs = t["off"][1:] - t["off"][:-1]
        assert len(np.unique(t["ids"])) == n and np.all(nobs >= 1) and np.all(nobs <= pi.MAX_OBS)
        assert np.all(t["start"] >= 0) and np.all(t["start"] + nobs - 1 <= pi.WINDOW)
        assert np.all(np.isfinite(t["depth"])) and np.all(np.isfinite(t["pts"])) and len(t["pts"]) == t["off"][-1]


def test_full_table():
    t, kinds = pi.table(pi.MAX_TRACKS, 10)
    q = kinds == pi.QUALIFIES
    assert 1024 <= q.sum() < 2048
    groups = q.reshape(-1, 64).sum(axis=1)
    assert (groups == 64).any() and (groups == 0).any()
    assert groups[1] == 64 and groups[2] == 0
    assert q[:1024].sum() not in (0, 1024) and q[1024:].sum() not in (0, 1024)      # both chunks of the kernel's walk compact


def test_all_none_and_edges():
    a, b = pi.all_or_none(1025, 10, True), pi.all_or_none(1025, 10, False)
    assert fp.qualifies(a["start"], a["off"][1:] - a["off"][:-1], a["depth"], 10).all()
    assert not fp.qualifies(b["start"], b["off"][1:] - b["off"][:-1], b["depth"], 10).any()
    e = pi.edge_depths(5)
    assert list(fp.qualifies(e["start"], e["off"][1:] - e["off"][:-1], e["depth"], 5)) == [False, False, False, True, True, True]
    assert [r for _, r, _ in pi.SIX] == [0, 1, 65, 1025, 2048, 64] and len({s for s, _, _ in pi.SIX}) == 6
    assert set(pi.SIZES) == {0, 1, 63, 64, 65, 1023, 1024, 1025, 2048} and set(pi.FRAME_COUNTS) == {0, 1, 2, 10}
