"""The batched structure-from-motion on the GPU (include/vio_sfm.h) against the numpy restatement (tests/sfm_reference.py), stage by
stage.

Stage 1 must give the same l, the same winning hypothesis and the same inlier mask, exactly; a fixture is used only if no error of
the winner (before or after the refit) lies within 1e-6 (relative) of the RANSAC gate, which the restatement reports as `margin`
(checked on the CPU for the windows below: the smallest margin is 1.4e-2, on the l = 5 window with inner tracks; no seed had to be dropped).  R, T and every stage-2 output
are held to 10x the restatement's own spread when each image point moves by one ulp (two such perturbations, measured in the test),
plus 1e-13 of the quantity's size: the rule of test_gpu_init.py, for the same reason (the conditioning of the triangulations and of
the reduced system varies by orders of magnitude between the windows).  Stage 2 is fed the restatement's stage-1 result, so a
stage-1 difference cannot hide in it.  PnP and BA iteration counts are compared too, except on a window where a one-ulp perturbation
already changes the restatement's count (at most one window in eight).  Two fixtures (syn_inner, syn_l5_inner) carry tracks that touch
neither frame l nor the newest frame, so that construct's last step (first and last observation, initial_sfm.cpp:196-210) is compared
and is part of the bitwise batch properties; tests/test_sfm_reference.py asserts on the CPU that they do (69 and 37 such tracks).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PX = 1.0 / 460.0


@pytest.fixture(scope="module")
def sfm_lib(vio, hip_lib):
    return vio.load_sfm()


def windows(vio):
    """(name, item): the two first windows without and with pixel noise, a window whose l is 5, F = 4 and F = VIO_SFM_MAX_FRAMES, a
    window with 20 % of the newest frame's points replaced by random outliers, and two windows (l = 0 and l = 5) with tracks that touch
    neither frame l nor the newest frame, which only construct's last step triangulates."""
    from vio_amd import stream as vs
    mh = dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))
    out = []
    for name, noise in (("syn", 0.0), ("syn_noisy", 0.1 * PX)):
        out.append((name, sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=10, pixel_noise=noise), list(range(11)))[0]))
    for name, noise in (("mh", 0.0), ("mh_noisy", 0.1 * PX)):
        st = vs.RealImuStream(mh, landmarks_per_frame=40, track_len=10, pixel_noise=noise)
        out.append((name, sr.window_item(st, list(range(11)))[0]))
    out.append(("syn_l5", sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=5, pixel_noise=0.1 * PX), list(range(11)))[0]))
    long = vs.SyntheticStream(landmarks_per_frame=30, track_len=15, pixel_noise=0.1 * PX, seed=2)
    out.append(("syn_F4", sr.window_item(long, list(range(4)))[0]))
    out.append(("syn_F16", sr.window_item(long, list(range(sr.MAX_FRAMES)))[0]))
    item = sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=10, pixel_noise=0.1 * PX, seed=4), list(range(11)))[0]
    out.append(("syn_outliers", with_outliers(item, 10, 0.2, seed=9)))
    for name, tl in (("syn_inner", 10), ("syn_l5_inner", 5)):
        item = sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=tl, pixel_noise=0.1 * PX, seed=6), list(range(11)))[0]
        out.append((name, with_inner_tracks(item, 0.3, seed=8)))
    return out


def with_inner_tracks(item, share, seed):
    """`share` of the tracks that start after frame 0 and have at least three observations lose their last observations so that they
    end before the newest frame (at least two stay).  With l = 0 such a track touches neither l nor F-1 and is left for the last
    step of construct (first and last observation, initial_sfm.cpp:196-210); with l = 5 so are the cut tracks that end before l."""
    rng = np.random.RandomState(seed)
    sf, off, pts = item["start_frame"], item["obs_offset"], item["pts"]
    F = item["n_frames"]
    nsf, noff, npts = [], [0], []
    for j in range(len(sf)):
        p = pts[off[j]:off[j + 1]]
        if sf[j] >= 1 and len(p) >= 3 and rng.rand() < share:
            p = p[:rng.randint(2, min(len(p), F - 1 - sf[j]) + 1)] if F - 1 - sf[j] >= 2 else p
        nsf.append(sf[j]); npts.extend(p); noff.append(noff[-1] + len(p))
    return dict(n_frames=F, start_frame=np.array(nsf, dtype=np.int32), obs_offset=np.array(noff, dtype=np.int64),
                pts=np.array(npts).reshape(-1, 2))


def with_outliers(item, frame, share, seed):
    """`share` of frame's observations replaced by uniform random points."""
    rng = np.random.RandomState(seed)
    sf, off = item["start_frame"], item["obs_offset"]
    n = off[1:] - off[:-1]
    tr = np.nonzero((sf <= frame) & (sf + n - 1 >= frame))[0]
    pick = rng.choice(tr, int(round(share * len(tr))), replace=False)
    pts = item["pts"].copy()
    pts[off[pick] + frame - sf[pick]] = rng.uniform(-0.5, 0.5, (len(pick), 2))
    return dict(item, pts=pts)


def _bar(spread, ref):
    ref = np.asarray(ref, dtype=np.float64)
    m = np.isfinite(ref)
    return 10.0 * float(np.max(spread)) + 1e-13 * max(1.0, float(np.abs(ref[m]).max()) if m.any() else 1.0)


def _close(got, ref, spread, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    m = ~np.isnan(ref)
    if not m.any():
        return
    bar = _bar(spread, ref)
    err = np.abs(got[m] - ref[m]).max()
    print("%-28s err %.3e  bar %.3e" % (what, err, bar))
    assert err <= bar, "%s: %.3e > %.3e" % (what, err, bar)


def _spread(ref, runs, keys):
    out = {}
    for k in keys:
        s = np.zeros_like(np.asarray(ref[k], dtype=np.float64))
        for p in runs:
            if p["status"] == ref["status"] and np.shape(p[k]) == np.shape(ref[k]):
                s = np.fmax(s, np.nan_to_num(np.abs(np.asarray(p[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)), nan=0.0))
        out[k] = s
    return out


def test_relative_pose_matches_restatement(vio, sfm_lib):
    ws = windows(vio)
    h = sfm_lib.create()
    got = h.relative_pose_batch([w[1] for w in ws])
    ls = set()
    for (name, item), g in zip(ws, got):
        ref = sr.relative_pose(item)
        assert ref["status"] == sr.OK, name
        assert ref["margin"] > 1e-6, (name, ref["margin"])       # else the fixture is not usable: take another seed
        rng = np.random.RandomState(5)
        runs = [sr.relative_pose(sr.perturb_ulp(item, rng)) for _ in range(2)]
        sp = _spread(ref, runs, ("R", "T", "parallax"))
        assert (g["status"], g["l"], g["hyp"]) == (ref["status"], ref["l"], ref["hyp"]), (name, g["l"], g["hyp"], ref["l"], ref["hyp"])
        assert g["n_corres"] == len(ref["mask"]) and np.array_equal(g["mask"], ref["mask"]), name
        assert g["n_inliers"] == ref["n_inliers"] and g["front"] == ref["front"], name
        assert np.array_equal(g["corres"], ref["corres"]), name
        for k in ("R", "T", "parallax"):
            _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))
        ls.add(ref["l"])
    assert 0 in ls and len(ls) > 1


STAGE2 = ("Q", "T", "points", "initial_cost", "final_cost")


def test_construct_matches_restatement(vio, sfm_lib):
    ws = windows(vio)
    h = sfm_lib.create()
    rels = [sr.relative_pose(w[1]) for w in ws]
    got = h.construct_batch([w[1] for w in ws], rels)
    left_out = remaining = 0
    for (name, item), rel, g in zip(ws, rels, got):
        ref = sr.construct(item, rel["l"], rel["R"], rel["T"])
        assert ref["status"] == sr.OK, (name, ref["status"])
        remaining += ref["n_remaining"] > 0
        rng = np.random.RandomState(6)
        runs = [sr.construct(sr.perturb_ulp(item, rng), rel["l"], rel["R"], rel["T"]) for _ in range(2)]
        sp = _spread(ref, runs, STAGE2)
        assert g["status"] == ref["status"] and g["fail_frame"] == ref["fail_frame"], (name, g["status"], g["fail_frame"])
        assert np.array_equal(g["state"], ref["state"]) and g["n_triangulated"] == int(ref["state"].sum()), name
        for k in STAGE2:
            _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))
        stable = all(np.array_equal(p["pnp_iterations"], ref["pnp_iterations"]) and p["ba_iterations"] == ref["ba_iterations"] for p in runs)
        print(name, "iterations", g["pnp_iterations"], g["ba_iterations"], "restatement", ref["pnp_iterations"], ref["ba_iterations"],
              "stable" if stable else "not stable under one ulp")
        if stable:
            assert np.array_equal(g["pnp_iterations"], ref["pnp_iterations"]), name
            assert g["ba_iterations"] == ref["ba_iterations"] and g["ba_converged"] == ref["ba_converged"], name
        else:
            left_out += 1
    assert left_out * 8 <= len(ws), left_out
    assert remaining >= 2           # the fixtures whose tracks reach construct's last step (first and last observation)


def test_both_stages_in_one_call(vio, sfm_lib):
    ws = windows(vio)
    h = sfm_lib.create()
    items = [w[1] for w in ws]
    both = h.sfm_batch(items)
    rel = h.relative_pose_batch(items)
    two = h.construct_batch(items, rel)
    for b, r, t in zip(both, rel, two):
        assert b["status"] == 0
        for k in ("l", "hyp", "n_inliers", "front"):
            assert b["rel"][k] == r[k]
        assert np.array_equal(b["rel"]["R"], r["R"]) and np.array_equal(b["rel"]["mask"], r["mask"])
        for k in ("Q", "T", "points", "state", "pnp_iterations"):
            assert np.array_equal(b[k], t[k], equal_nan=True), k
        assert b["final_cost"] == t["final_cost"] and b["ba_iterations"] == t["ba_iterations"]
    init_items = vio.sfm_items_to_init_items(both, np.eye(3), [[None] * 10 for _ in both])
    assert all(it is not None and it["R"].shape[1:] == (3, 3) for it in init_items)


def _bits(d):
    keys = ("status", "fail_frame", "Q", "T", "points", "state", "pnp_iterations", "ba_iterations", "initial_cost", "final_cost")
    out = [np.asarray(d[k]).tobytes() for k in keys]
    r = d["rel"]
    return out + [np.asarray(r[k]).tobytes() for k in ("status", "l", "hyp", "R", "T", "mask", "corres", "parallax")]


def failing_items(vio):
    """A window with too few correspondences (relativePose fails) and one with a NaN point."""
    from vio_amd import stream as vs
    few = sr.window_item(vs.SyntheticStream(landmarks_per_frame=15, track_len=1, pixel_noise=0.1 * PX), list(range(11)))[0]
    nan = sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=10, pixel_noise=0.1 * PX), list(range(11)))[0]
    pts = nan["pts"].copy()
    pts[17, 1] = np.nan
    return few, dict(nan, pts=pts)


def test_batch_properties(vio, sfm_lib):
    ws = windows(vio)
    h = sfm_lib.create()
    items = [w[1] for w in ws]
    alone = [h.sfm_batch([it])[0] for it in items]
    big = [items[k % len(items)] for k in range(64)]
    out64 = h.sfm_batch(big)
    again = h.sfm_batch(big)
    for k in range(64):
        assert _bits(out64[k]) == _bits(alone[k % len(items)]), k          # alone, in a batch of 64, at several positions
        assert _bits(out64[k]) == _bits(again[k]), k                        # two calls
    few, nan = failing_items(vio)
    mixed = [items[0], nan, items[1], few, items[2]]
    out = h.sfm_batch(mixed)
    assert [o["status"] for o in out] == [0, sr.NOT_FINITE, 0, sr.FAIL_RELATIVE_POSE, 0]
    assert out[1]["rel"]["status"] == sr.NOT_FINITE and np.all(np.isnan(out[1]["Q"])) and np.all(np.isnan(out[1]["points"]))
    assert out[3]["rel"]["l"] == -1 and np.all(np.isnan(out[3]["T"])) and not out[3]["state"].any()
    for k, j in ((0, 0), (2, 1), (4, 2)):
        assert _bits(out[k]) == _bits(alone[j])
    ref = sr.sfm(few)
    assert ref["status"] == sr.FAIL_RELATIVE_POSE and np.array_equal(out[3]["rel"]["corres"], ref["rel"]["corres"])


def test_pnp_failure_is_reported(vio, sfm_lib):
    """A frame with fewer than 10 PnP points: the status and the frame of the restatement."""
    item = sparse_frame_item(vio)
    rel = sr.relative_pose(item)
    ref = sr.construct(item, rel["l"], rel["R"], rel["T"])
    assert ref["status"] == sr.FAIL_PNP and ref["fail_frame"] >= 0
    g = sfm_lib.create().construct_batch([item], [rel])[0]
    assert (g["status"], g["fail_frame"]) == (ref["status"], ref["fail_frame"])
    assert np.all(np.isnan(g["Q"])) and np.all(np.isnan(g["points"]))


def sparse_frame_item(vio):
    """The first synthetic window with the tracks that span frame 4 cut in front of it, all but 9: l becomes 5 and frame 4's PnP, the
    first of the backward chain, sees 9 points."""
    from vio_amd import stream as vs
    item = sr.window_item(vs.SyntheticStream(landmarks_per_frame=30, track_len=10, pixel_noise=0.1 * PX), list(range(11)))[0]
    return cut_frame(item, 4, 9)


def cut_frame(item, frame, keep):
    """Tracks that span `frame` and do not reach the newest frame are cut in front of it, and of those that do only `keep` stay whole:
    the others lose everything from `frame` on."""
    sf, off, pts = item["start_frame"], item["obs_offset"], item["pts"]
    F = item["n_frames"]
    nsf, noff, npts, whole = [], [0], [], 0
    for j in range(len(sf)):
        n = off[j + 1] - off[j]
        p = pts[off[j]:off[j + 1]]
        if sf[j] <= frame <= sf[j] + n - 1:
            if sf[j] + n - 1 >= F - 1 and sf[j] == 0 and whole < keep:
                whole += 1
            elif sf[j] < frame:
                p = p[:frame - sf[j]]
            else:
                continue
        nsf.append(sf[j]); npts.extend(p); noff.append(noff[-1] + len(p))
    return dict(n_frames=F, start_frame=np.array(nsf, dtype=np.int32), obs_offset=np.array(noff, dtype=np.int64),
                pts=np.array(npts).reshape(-1, 2))


def test_count_zero_and_bad_arguments(vio, sfm_lib):
    h = sfm_lib.create()
    assert h.sfm_batch([]) == [] and h.relative_pose_batch([]) == []
    item = windows(vio)[0][1]
    good = h.sfm_batch([item])[0]
    for bad in (dict(item, n_frames=2), dict(item, n_frames=sr.MAX_FRAMES + 1), dict(item, n_frames=5)):
        with pytest.raises(vio.VioError) as e:
            h.sfm_batch([item, bad])
        assert e.value.status == -1 and "window 1" in str(e.value)
    with pytest.raises(vio.VioError):
        h.set_config(ransac_hypotheses=0)
    with pytest.raises(vio.VioError):
        h.construct_batch([item], [dict(status=0, l=10, R=np.eye(3), T=np.ones(3))])
    fn = sfm_lib.fn["relative_pose_batch"]
    assert fn(h.h, C.c_int32(-1), None, None, None) == -1 and fn(h.h, C.c_int32(1), None, None, None) == -1
    assert _bits(h.sfm_batch([item])[0]) == _bits(good)         # the handle is unharmed
    h.set_config(seed=3, ransac_hypotheses=64)
    other = h.sfm_batch([item])[0]
    assert other["status"] == 0 and other["rel"]["hyp"] < 64
