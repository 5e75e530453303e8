"""numpy restatement of include/vio_flow_back.h: the forward-backward check of the Lucas-Kanade tracker, over tests/flow_reference.py
(DESIGN.md section 36).

    verdict(back_ok, p, b, max_dist)      the status of one keypoint and the squared distance it compares
    track_back(img_prev, img_next, pts)   the forward pass, the backward pass of the keypoints that are OK forwards, the verdicts
    fixture()                             the 96 x 72 pair and its 140 keypoints that reach every outcome, in both modes

Every product and sum is one rounded double operation; positions are float32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as fr  # noqa: E402

OK, NOT_FINITE, FAIL_LOST, FAIL_BORDER = fr.OK, fr.NOT_FINITE, fr.FAIL_LOST, fr.FAIL_BORDER
FAIL_BACK_LOST, FAIL_BACK_FAR, BACK_NOT_RUN = 3, 4, -1
DEFAULT_MAX_DIST = 0.5


def verdict(back_ok, p, b, max_dist=DEFAULT_MAX_DIST):
    """(status, d2) of a keypoint at p (float32 pair) whose backward pass ended at b: d2 is formed whenever the pass ran."""
    with np.errstate(all="ignore"):
        dx = np.float64(np.float32(b[0])) - np.float64(np.float32(p[0]))
        dy = np.float64(np.float32(b[1])) - np.float64(np.float32(p[1]))
        d2 = dx * dx + dy * dy
        lim = np.float64(max_dist) * np.float64(max_dist)
    if not back_ok:
        return FAIL_BACK_LOST, float(d2)
    return (OK if d2 <= lim else FAIL_BACK_FAR), float(d2)


def track_back(img_prev, img_next, pts, guess=None, levels=4, back_levels=0, max_dist=DEFAULT_MAX_DIST, order="wave64", **cfg):
    """dict(next_pts, status, iterations, cost, back_pts, back_status, back_iterations, back_cost, back_d2) of the keypoints pts;
    cfg: half_patch, max_iter, inverse, border, early_stop of flow_reference.multi_level."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    bl = int(back_levels) if back_levels else int(levels)
    assert 1 <= bl <= levels
    nxt, st, its, cost = fr.multi_level(img_prev, img_next, pts, guess=guess, levels=levels, order=order, **cfg)
    st = st.copy()
    bpts = np.full((n, 2), np.nan, dtype=np.float32)
    bst = np.full(n, BACK_NOT_RUN, dtype=np.int32)
    bits = np.zeros(n, dtype=np.int32)
    bcost = np.full(n, np.nan)
    d2 = np.full(n, np.nan)
    k = np.nonzero(st == OK)[0]
    if len(k):
        bcfg = dict(cfg)
        bcfg["border"] = 0
        b, s, i, c = fr.multi_level(img_next, img_prev, nxt[k], guess=pts[k], levels=bl, order=order, **bcfg)
        assert not np.any(s == NOT_FINITE)
        bpts[k], bits[k], bcost[k] = b, i, c
        bst[k] = np.where(s == FAIL_LOST, FAIL_LOST, OK)
        for j, r in enumerate(k):
            st[r], d2[r] = verdict(s[j] != FAIL_LOST, pts[r], b[j], max_dist)
    return dict(next_pts=nxt, status=st, iterations=its, cost=cost, back_pts=bpts, back_status=bst, back_iterations=bits, back_cost=bcost,
                back_d2=d2)


FIXTURE_LEVELS = 3


def fixture():
    """(a, b, pts): a 96 x 72 texture, the same texture shifted by (3, 2) with its left 28 columns and top 20 rows replaced by another
    texture (points there track somewhere and do not come back), and 140 keypoints on a grid."""
    a = fr.texture(96, 72, 5)
    b = fr.texture(96, 72, 5, shift=(3.0, 2.0)).copy()
    other = fr.texture(96, 72, 105, smooth=1.5)
    b[:, :28] = other[:, :28]
    b[:20, :] = other[:20, :]
    xs, ys = np.arange(5, 91, 6.5), np.arange(5, 67, 6.25)
    pts = np.array([(x + 0.3, y + 0.6) for x in xs for y in ys], dtype=np.float32)
    assert pts.shape == (140, 2)
    return a, b, pts


_CACHE = {}


def fixture_reference(inverse, back_levels):
    """track_back of the fixture, computed once per (inverse, back_levels) and shared: do not change what it returns."""
    key = (int(inverse), int(back_levels))
    if key not in _CACHE:
        a, b, pts = fixture()
        _CACHE[key] = track_back(a, b, pts, levels=FIXTURE_LEVELS, back_levels=back_levels, inverse=int(inverse))
    return _CACHE[key]


def counts(ref):
    st, bst = ref["status"], ref["back_status"]
    return dict(forward_ok=int(np.sum(bst != BACK_NOT_RUN)), forward_lost=int(np.sum(st == FAIL_LOST)), back_lost=int(np.sum(st == FAIL_BACK_LOST)),
                back_far=int(np.sum(st == FAIL_BACK_FAR)), kept=int(np.sum(st == OK)))
