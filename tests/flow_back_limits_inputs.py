"""The inputs of the forward-backward check's tests at its limits and their cached restatements (tests/test_flow_back_limits_inputs_cpu.py
holds them to what the GPU tests assume, tests/test_gpu_flow_back_limits.py and tests/test_gpu_front_back_limits.py run them on the
device).  No tests in here.  Every restatement is tests/flow_back_reference.track_back, computed once and shared:
do not change what these functions return.

    full(inverse)           front_limits_inputs.image(0) -> image(1) (192 x 144), the 1024 rows of front_limits_inputs.seeded(1024), under
                            FULL_CFG (levels 2, back_levels 2, half_patch 2, border 1: what tests/test_gpu_front.py's Rig hands the
                            tracker).  A keypoint is one wavefront's work and depends on no other keypoint, so the restatement of the
                            first n rows is the first n rows of this one: prefix(ref, n)
    settings()              the named cases on flow_back_reference.fixture(): the patch sizes with idle lanes, a ragged second term,
                            7 and 16 terms a lane; back_levels 1 under 3 and 4, 4 under 4, 1 under 1; a forward guess; max_iter 1;
                            early_stop off and on
    small()                 a 33 x 25 pair, 108 grid points, half_patch 1, 4, 5 under (levels, back_levels) (1, 1), (3, 1), (3, 3)
    strided()               the fixture pair in arrays seven bytes wider than the image; the restatement is the contiguous pair's
    mixed(back_levels, inverse)   three items of different sizes under levels 2, half_patch 2
    boundary_rows(ref)      the rows whose backward pass came back with 0 < d2 < 1, each with the doubles just below, at and just above
                            sqrt(d2); verdict_at(d2, m) is the header's verdict for max_dist = m, in numpy doubles
    restate(case)           the cached restatement of a settings(), small() or mixed() case

early_stop: include/vio_flow.h's default is 0, so the fixture's restatement in tests/test_gpu_flow_back.py already runs with it off; the
case "early_stop 0" restates that and "early_stop 1" is the one that no other test runs with the check on.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_reference as fb  # noqa: E402
import flow_reference as fr  # noqa: E402
import front_limits_inputs as fl  # noqa: E402

CAP, WAVE = fl.CAP, fl.WAVE
FULL_CFG = dict(levels=2, back_levels=2, half_patch=2, border=1)
GUESS_SHIFT = (2.5, 1.5)
PAD = 7                                             # strided(): the bytes a row is wider than the image
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- the full table ------------------------------------------------------------------------------------------------
def full_inputs():
    """(img_prev, img_next, pts (1024, 2) float32)."""
    return np.ascontiguousarray(fl.image(0)), np.ascontiguousarray(fl.image(1)), fl.seeded(CAP)[0]


def full(inverse):
    """track_back of the 1024 rows, once per mode (4 to 7 s of numpy)."""
    return _once(("full", int(inverse)), lambda: fb.track_back(*full_inputs(), inverse=int(inverse), **FULL_CFG))


def prefix(ref, n, lo=0):
    """Rows lo .. n - 1 of a restatement."""
    return {k: v[lo:n] for k, v in ref.items()}


def failed_groups(ref):
    """The 64-row groups of a restatement that hold at least one row that failed the check."""
    st = ref["status"]
    return sorted(set((np.nonzero((st == fb.FAIL_BACK_LOST) | (st == fb.FAIL_BACK_FAR))[0] // WAVE).tolist()))


def back_info(ref):
    """vio_frame_read_back_info's three counts of a restatement."""
    c = fb.counts(ref)
    return dict(n_checked=c["forward_ok"], n_back_lost=c["back_lost"], n_back_far=c["back_far"])


# ---- named settings on the fixture ---------------------------------------------------------------------------------
def _case(name, levels, back_levels, inverse=0, guess=False, **flow):
    return dict(name=name, levels=levels, back_levels=back_levels, inverse=inverse, guess=guess, flow=flow)


def settings():
    """The cases: dicts of name, levels, back_levels, inverse, guess (True: pts + GUESS_SHIFT) and flow (the other arguments of
    FlowHandle.set_config)."""
    return [
        _case("half_patch 16, 2/2", 2, 2, half_patch=16),
        _case("half_patch 16, 2/1, inverse", 2, 1, inverse=1, half_patch=16),
        _case("half_patch 10, 3/1", 3, 1, half_patch=10),
        _case("half_patch 1, 3/3", 3, 3, half_patch=1),
        _case("guess, 3/2", 3, 2, guess=True),
        _case("guess, 1/1, inverse", 1, 1, inverse=1, guess=True),
        _case("max_iter 1, 3/2", 3, 2, max_iter=1),
        _case("early_stop 0, 3/2", 3, 2, early_stop=0),
        _case("early_stop 1, 3/2", 3, 2, early_stop=1),
        _case("4/4", 4, 4),
        _case("4/1, inverse", 4, 1, inverse=1),
        _case("half_patch 5, 3/2", 3, 2, half_patch=5),
        _case("half_patch 5, 3/2, inverse", 3, 2, inverse=1, half_patch=5),
    ]


# what the issue's table gives for these cases: (OK forwards, kept, lost backwards, far), asserted as computed on a CPU
SETTINGS_COUNTS = {
    "half_patch 16, 2/2": (70, 27, 2, 41), "half_patch 16, 2/1, inverse": (70, 29, 0, 41), "half_patch 10, 3/1": (108, 37, 12, 59),
    "half_patch 1, 3/3": (105, 50, 14, 41), "guess, 3/2": (129, 57, 9, 63), "guess, 1/1, inverse": (124, 44, 6, 74),
    "max_iter 1, 3/2": (140, 59, 0, 81), "early_stop 0, 3/2": (132, 64, 7, 61), "4/4": (132, 63, 7, 62), "4/1, inverse": (132, 64, 3, 65),
}


def settings_inputs(case):
    """(img_prev, img_next, pts, guess or None) of a settings() case."""
    a, b, pts = fb.fixture()
    g = (pts + np.array(GUESS_SHIFT, dtype=np.float32)).astype(np.float32) if case["guess"] else None
    return a, b, pts, g


# ---- the small pair ------------------------------------------------------------------------------------------------
SMALL_W, SMALL_H = 33, 25


def small_inputs():
    """(img_prev, img_next, pts (108, 2)): the 33 x 25 pair of tests/test_gpu_flow_back.py's three-item call and a grid over all of it;
    the points whose patch leaves the image are FAIL_LOST forwards and get the backward row of a pass that did not run."""
    sa, sb = fr.texture(SMALL_W, SMALL_H, 8), fr.texture(SMALL_W, SMALL_H, 8, shift=(0.6, -0.4))
    pts = np.array([(x, y) for x in np.arange(2.0, 30.0, 2.5) for y in np.arange(2.0, 23.0, 2.5)], dtype=np.float32)
    assert pts.shape == (108, 2)
    return sa, sb, pts


def small():
    return [_case("33 x 25, half_patch %d, %d/%d%s" % (hp, lv, bl, ", inverse" if inv else ""), lv, bl, inverse=inv, half_patch=hp)
            for hp in (1, 4, 5) for lv, bl in ((1, 1), (3, 1), (3, 3)) for inv in (0, 1)]


def restate(case):
    """The cached restatement of a settings(), small() or mixed() case."""
    def make():
        if case["name"].startswith("33 x 25"):
            a, b, pts = small_inputs()
            g = None
        else:
            a, b, pts, g = settings_inputs(case)
        return fb.track_back(a, b, pts, guess=g, levels=case["levels"], back_levels=case["back_levels"], inverse=case["inverse"], **case["flow"])
    return _once(("case", case["name"]), make)


# ---- rows of another stride than the width ---------------------------------------------------------------------------
def strided():
    """(img_prev, img_next, pts): views of the fixture pair whose rows are PAD bytes apart more than they are wide, the gap filled with
    255.  The restatement is fixture_reference's."""
    def make():
        a, b, pts = fb.fixture()
        out = []
        for img in (a, b):
            wide = np.full((img.shape[0], img.shape[1] + PAD), 255, dtype=np.uint8)
            wide[:, :img.shape[1]] = img
            out.append(wide[:, :img.shape[1]])
        return out[0], out[1], pts
    return _once("strided", make)


# ---- items of different sizes in one call ----------------------------------------------------------------------------
MIXED_CFG = dict(levels=2, half_patch=2, border=1)
MIXED_ROWS = 65                                     # of the 192 x 144 pair's 1024


def mixed_items():
    """[(img_prev, img_next, pts)] of 192 x 144, 96 x 72 and 33 x 25."""
    a, b, pts = full_inputs()
    return [(a, b, pts[:MIXED_ROWS])] + [fb.fixture(), small_inputs()]


def mixed(back_levels, inverse):
    """The restatements of mixed_items() under MIXED_CFG."""
    def make():
        if int(back_levels) == FULL_CFG["back_levels"]:
            first = prefix(full(inverse), MIXED_ROWS)
        else:
            first = fb.track_back(*mixed_items()[0], back_levels=back_levels, inverse=int(inverse), **MIXED_CFG)
        return [first] + [fb.track_back(*it, back_levels=back_levels, inverse=int(inverse), **MIXED_CFG) for it in mixed_items()[1:]]
    return _once(("mixed", int(back_levels), int(inverse)), make)


# ---- the verdict next to its boundary --------------------------------------------------------------------------------
def verdict_at(d2, m):
    """include/vio_flow_back.h's verdict of a backward pass that came back, for max_dist = m: both sides in doubles."""
    d2, m = np.float64(d2), np.float64(m)
    return fb.OK if d2 <= m * m else fb.FAIL_BACK_FAR


def boundary_rows(ref):
    """[(row, (m-, m0, m+))] of the rows whose backward pass came back with 0 < d2 < 1: the doubles around sqrt(d2)."""
    out = []
    with np.errstate(invalid="ignore"):
        rows = np.nonzero((ref["back_status"] == fb.OK) & (ref["back_d2"] > 0.0) & (ref["back_d2"] < 1.0))[0]
    for r in rows:
        m0 = np.sqrt(np.float64(ref["back_d2"][r]))
        out.append((int(r), (float(np.nextafter(m0, 0.0)), float(m0), float(np.nextafter(m0, np.inf)))))
    return out


def has_exact(d2, ms):
    """True if one of the doubles ms squares to d2 exactly: the row that tells <= from <."""
    return any(np.float64(m) * np.float64(m) == np.float64(d2) for m in ms)


def boundary_pick(ref, n=3):
    """n boundary rows whose three max_dist values give both verdicts, those with an exact square first."""
    rows = [(r, ms) for r, ms in boundary_rows(ref) if len({verdict_at(ref["back_d2"][r], m) for m in ms}) == 2]
    rows.sort(key=lambda x: (not has_exact(ref["back_d2"][x[0]], x[1]), x[0]))
    return rows[:n]
