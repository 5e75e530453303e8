"""The batched structure-from-motion at the limits of include/vio_sfm.h and at other settings than the defaults, against the numpy
restatement (tests/sfm_reference.py).  The rules are those of tests/test_gpu_sfm.py: stage 1 must reproduce status, l, the winning
hypothesis, the counts, the per-candidate correspondences and the inlier mask exactly; R, T, parallax and every stage-2 output are
held to 10x the restatement's own spread under two one-ulp perturbations plus 1e-13 of the quantity's size; stage 2 is fed the
restatement's stage-1 result; a fixture is usable only if the restatement's margin to the RANSAC gate is above 1e-6.

What test_gpu_sfm.py leaves out and this file runs:
  - hypothesis counts 1, 255, 256, 257, 1000 and VIO_SFM_MAX_HYPOTHESES: above 256 a thread of k_sfm_relpose fits more than one
    hypothesis and the tie-break across threads sees candidates that are not their thread's index.  The restatement's winner lies at
    or above 256 on syn_F16 (846) and syn_outliers (421) with 1000 hypotheses (measured on the CPU), so no extra window was needed;
    the test asserts that some winner does;
  - the sampling hash with seeds 3 and 0xFFFFFFFF;
  - windows of 1 100, 4 000 and exactly VIO_SFM_MAX_TRACKS tracks (the scratch offsets, the int32 casts of obs_offset, the serial
    gathers on thread 0, the TR / OB / PC strides), F = 3 (one candidate frame, a bundle adjustment with one free rotation), a window
    without tracks, a batch whose windows differ by three orders of magnitude in size, and the refusal of 4 097 tracks.
Measured on the CPU: the margins of the new windows are 1.1e-1 (1 100 tracks), 4.5e-4 (4 000 and 4 096 tracks) and 5.1e-3 (F = 3).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_reference as sr  # noqa: E402
from test_gpu_sfm import PX, STAGE2, _bits, _close, _spread, windows  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_TRACKS = 4096
MAX_HYPOTHESES = 4096
CONFIGS = [(1, 0), (255, 0), (256, 0), (257, 0), (1000, 0), (MAX_HYPOTHESES, 0), (128, 3), (128, 0xFFFFFFFF)]
CONFIG_IDS = ["hyps%d_seed%s" % (h, s if s < 10 else hex(s)) for h, s in CONFIGS]
LIMIT_NAMES = ["tracks1100_F11", "tracks4000_F16", "tracks4096_F16", "tracks90_F3"]


@pytest.fixture(scope="module")
def sfm_lib(vio, hip_lib):
    return vio.load_sfm()


@pytest.fixture(scope="module")
def default_windows(vio):
    return windows(vio)


def padded_to(item, n_tracks, seed):
    """item with two-observation tracks appended until it has n_tracks: each is a copy of two consecutive observations, in the middle
    frames of the window, of a track drawn at random.  They reach neither frame 0 nor the newest frame, so stage 1 does not see them
    and construct's last step (first and last observation) triangulates them."""
    rng = np.random.RandomState(seed)
    sf, off = np.asarray(item["start_frame"]), np.asarray(item["obs_offset"])
    pts = np.asarray(item["pts"], dtype=np.float64).reshape(-1, 2)
    F = item["n_frames"]
    n = off[1:] - off[:-1]
    nsf, noff, npts = list(sf), list(off), [pts]
    while len(nsf) < n_tracks:
        j, f = rng.randint(len(sf)), rng.randint(F // 4, 3 * F // 4)
        if sf[j] <= f and sf[j] + n[j] - 1 >= f + 1:
            o = off[j] + f - sf[j]
            nsf.append(f); npts.append(pts[o:o + 2]); noff.append(noff[-1] + 2)
    return dict(n_frames=F, start_frame=np.array(nsf, dtype=np.int32), obs_offset=np.array(noff, dtype=np.int64),
                pts=np.concatenate(npts).reshape(-1, 2))


def empty_item(F=11):
    return dict(n_frames=F, start_frame=np.zeros(0, dtype=np.int32), obs_offset=np.zeros(1, dtype=np.int64), pts=np.zeros((0, 2)))


@pytest.fixture(scope="module")
def limit_windows(vio):
    """name -> item, built once: (landmarks per frame, track length, F) = (100, 10, 11), (250, 15, 16), the latter padded to exactly
    VIO_SFM_MAX_TRACKS tracks, (30, 15, 3) of stream seed 2, and a window without tracks."""
    from vio_amd import stream as vs

    def make(L, T, F, seed=0):
        return sr.window_item(vs.SyntheticStream(landmarks_per_frame=L, track_len=T, pixel_noise=0.1 * PX, seed=seed), list(range(F)))[0]

    out = {"tracks1100_F11": make(100, 10, 11), "tracks4000_F16": make(250, 15, 16), "tracks90_F3": make(30, 15, 3, seed=2),
           "tracks0_F11": empty_item()}
    out["tracks4096_F16"] = padded_to(out["tracks4000_F16"], MAX_TRACKS, seed=12)
    want = {"tracks1100_F11": (1100, 6600), "tracks4000_F16": (4000, 34000), "tracks4096_F16": (4096, 34192), "tracks90_F3": (90, 180),
            "tracks0_F11": (0, 0)}
    for name, (nt, nobs) in want.items():
        assert (len(out[name]["start_frame"]), len(out[name]["pts"])) == (nt, nobs), name
    return out


@pytest.fixture(scope="module")
def stage1_refs():
    """The restatement's stage 1 per (window, hypotheses, seed), computed once."""
    return {}


def stage1_ref(cache, name, item, hyps, seed):
    key = (name, hyps, seed)
    if key not in cache:
        cache[key] = sr.relative_pose(item, dict(ransac_hypotheses=hyps, seed=seed))
    return cache[key]


def check_stage1(name, item, g, ref, cfg):
    """test_gpu_sfm.test_relative_pose_matches_restatement's comparison of one window."""
    assert ref["status"] == sr.OK, name
    assert ref["margin"] > 1e-6, (name, ref["margin"])       # else the fixture is not usable
    rng = np.random.RandomState(5)
    runs = [sr.relative_pose(sr.perturb_ulp(item, rng), cfg) for _ in range(2)]
    sp = _spread(ref, runs, ("R", "T", "parallax"))
    print("%-28s l %d hyp %d inliers %d of %d margin %.2e" % (name, ref["l"], ref["hyp"], ref["n_inliers"], len(ref["mask"]), ref["margin"]))
    assert (g["status"], g["l"], g["hyp"]) == (ref["status"], ref["l"], ref["hyp"]), (name, g["l"], g["hyp"], ref["l"], ref["hyp"])
    assert g["n_corres"] == len(ref["mask"]) and np.array_equal(g["mask"], ref["mask"]), name
    assert g["n_inliers"] == ref["n_inliers"] and g["front"] == ref["front"], name
    assert np.array_equal(g["corres"], ref["corres"]), name
    for k in ("R", "T", "parallax"):
        _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))


@pytest.mark.parametrize("hyps,seed", CONFIGS, ids=CONFIG_IDS)
def test_relative_pose_at_other_settings(sfm_lib, default_windows, stage1_refs, hyps, seed):
    """relative_pose_batch over the ten windows of test_gpu_sfm.py with `hyps` hypotheses and the sampling seed `seed`, against
    sr.relative_pose with the same configuration."""
    h = sfm_lib.create()
    h.set_config(seed=seed, ransac_hypotheses=hyps)
    got = h.relative_pose_batch([w[1] for w in default_windows])
    cfg = dict(ransac_hypotheses=hyps, seed=seed)
    for (name, item), g in zip(default_windows, got):
        check_stage1("%s[%d,%d]" % (name, hyps, seed), item, g, stage1_ref(stage1_refs, name, item, hyps, seed), cfg)


def test_a_hypothesis_beyond_the_first_256_wins(default_windows, stage1_refs):
    """The comparisons above show the strided branch of k_sfm_relpose's hypothesis loop to decide something only if, for some window
    and some count above 256, the restatement's winner is a hypothesis a thread reaches in its second or a later turn."""
    late = [(name, hyps, stage1_ref(stage1_refs, name, item, hyps, seed)["hyp"]) for hyps, seed in CONFIGS if hyps > 256
            for name, item in default_windows]
    late = [x for x in late if x[2] >= 256]
    print(late)
    assert late


LEFT_OUT = {}


@pytest.mark.parametrize("name", LIMIT_NAMES)
def test_both_stages_at_the_size_limits(sfm_lib, limit_windows, name):
    """Stage 1, and stage 2 from the restatement's stage 1, of one large or small window against the restatement.  The iteration
    counts are compared unless a one-ulp perturbation changes the restatement's own (at most one window in eight of LIMIT_NAMES)."""
    item = limit_windows[name]
    h = sfm_lib.create()
    rel = sr.relative_pose(item)
    check_stage1(name, item, h.relative_pose_batch([item])[0], rel, None)
    g = h.construct_batch([item], [rel])[0]
    ref = sr.construct(item, rel["l"], rel["R"], rel["T"])
    assert ref["status"] == sr.OK, (name, ref["status"])
    rng = np.random.RandomState(6)
    runs = [sr.construct(sr.perturb_ulp(item, rng), rel["l"], rel["R"], rel["T"]) for _ in range(2)]
    sp = _spread(ref, runs, STAGE2)
    assert g["status"] == ref["status"] and g["fail_frame"] == ref["fail_frame"], (name, g["status"], g["fail_frame"])
    assert np.array_equal(g["state"], ref["state"]) and g["n_triangulated"] == int(ref["state"].sum()), name
    for k in STAGE2:
        _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))
    stable = all(np.array_equal(p["pnp_iterations"], ref["pnp_iterations"]) and p["ba_iterations"] == ref["ba_iterations"] for p in runs)
    print(name, "iterations", g["pnp_iterations"], g["ba_iterations"], "restatement", ref["pnp_iterations"], ref["ba_iterations"],
          "remaining", ref["n_remaining"], "stable" if stable else "not stable under one ulp")
    LEFT_OUT[name] = not stable
    if stable:
        assert np.array_equal(g["pnp_iterations"], ref["pnp_iterations"]), name
        assert g["ba_iterations"] == ref["ba_iterations"] and g["ba_converged"] == ref["ba_converged"], name
    assert sum(LEFT_OUT.values()) * 8 <= len(LIMIT_NAMES), LEFT_OUT
    if name == "tracks4096_F16":
        assert ref["n_remaining"] == MAX_TRACKS - 4000          # the appended tracks reach construct's last step
    if name == "tracks90_F3":
        assert rel["l"] == 0 and ref["ba_iterations"] > 0


def test_4097_tracks_are_refused_and_nothing_is_written(vio, sfm_lib, default_windows, limit_windows):
    from vio_amd.sfm import VioSfmRelResult, VioSfmResult, _Packed
    h = sfm_lib.create()
    syn = default_windows[0][1]
    good = h.sfm_batch([syn])[0]
    over = padded_to(limit_windows["tracks4000_F16"], MAX_TRACKS + 1, seed=12)
    assert len(over["start_frame"]) == MAX_TRACKS + 1
    for call in (h.sfm_batch, h.relative_pose_batch):
        with pytest.raises(vio.VioError) as e:
            call([syn, over])
        assert e.value.status == -1 and "window 1" in str(e.value) and "n_tracks" in str(e.value)
    pk = _Packed([syn, over])
    rel, res = (VioSfmRelResult * 2)(), (VioSfmResult * 2)()
    for r in list(rel) + list(res):
        r.status = 77
    mask = np.full(pk.total, 9, dtype=np.uint8)
    state = np.full(pk.total, 9, dtype=np.uint8)
    points = np.full((pk.total, 3), 5.0)
    fn = sfm_lib.fn
    assert fn["batch"](h.h, C.c_int32(2), C.addressof(pk.items), C.addressof(rel), mask.ctypes.data, C.addressof(res), points.ctypes.data,
                       state.ctypes.data) == -1
    assert fn["relative_pose_batch"](h.h, C.c_int32(2), C.addressof(pk.items), C.addressof(rel), mask.ctypes.data) == -1
    assert fn["construct_batch"](h.h, C.c_int32(2), C.addressof(pk.items), C.addressof(rel), C.addressof(res), points.ctypes.data,
                                 state.ctypes.data) == -1
    assert b"window 1" in fn["last_error"](h.h)
    assert all(r.status == 77 for r in list(rel) + list(res))
    assert np.all(mask == 9) and np.all(state == 9) and np.all(points == 5.0)
    assert _bits(h.sfm_batch([syn])[0]) == _bits(good)         # the handle is unharmed


def test_a_window_without_tracks(sfm_lib, limit_windows):
    item = limit_windows["tracks0_F11"]
    ref = sr.sfm(item)
    assert ref["status"] == sr.FAIL_RELATIVE_POSE and ref["rel"]["l"] == -1
    h = sfm_lib.create()
    g = h.sfm_batch([item])[0]
    assert g["status"] == sr.FAIL_RELATIVE_POSE and g["fail_frame"] == -1
    r = g["rel"]
    assert (r["status"], r["l"], r["hyp"], r["n_corres"], r["n_inliers"], r["front"]) == (sr.FAIL_RELATIVE_POSE, -1, -1, 0, 0, 0)
    assert np.array_equal(r["corres"], ref["rel"]["corres"]) and np.array_equal(r["parallax"], ref["rel"]["parallax"])
    assert np.all(np.isnan(r["R"])) and np.all(np.isnan(r["T"])) and r["mask"].shape == (0,)
    assert g["Q"].shape == (11, 4) and np.all(np.isnan(g["Q"])) and g["T"].shape == (11, 3) and np.all(np.isnan(g["T"]))
    assert g["points"].shape == (0, 3) and g["state"].shape == (0,) and g["n_triangulated"] == 0
    assert np.isnan(g["initial_cost"]) and np.isnan(g["final_cost"]) and g["ba_iterations"] == 0
    rel = h.relative_pose_batch([item])[0]
    assert rel["status"] == sr.FAIL_RELATIVE_POSE and rel["l"] == -1
    two = h.construct_batch([item], [rel])[0]
    assert two["status"] == sr.FAIL_RELATIVE_POSE and np.all(np.isnan(two["Q"])) and np.all(np.isnan(two["T"]))


def test_a_batch_of_very_different_windows(sfm_lib, default_windows, limit_windows):
    """[4 096 tracks, none, F = 3, syn, 4 000 tracks, syn_F4] in one call: every window's bits are those it has alone (the scratch
    and output offsets accumulate over the batch), and the reversed batch gives the same bits."""
    by_name = dict(default_windows)
    items = [limit_windows["tracks4096_F16"], limit_windows["tracks0_F11"], limit_windows["tracks90_F3"], by_name["syn"],
             limit_windows["tracks4000_F16"], by_name["syn_F4"]]
    h = sfm_lib.create()
    alone = [h.sfm_batch([it])[0] for it in items]
    assert [a["status"] for a in alone] == [0, sr.FAIL_RELATIVE_POSE, 0, 0, 0, 0]
    out = h.sfm_batch(items)
    back = h.sfm_batch(items[::-1])[::-1]
    for k in range(len(items)):
        assert _bits(out[k]) == _bits(alone[k]), k
        assert _bits(back[k]) == _bits(alone[k]), k
