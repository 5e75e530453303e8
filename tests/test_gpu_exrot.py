"""libvio_exrot_hip.so (include/vio_exrot.h) against the numpy restatement (tests/exrot_reference.py) on directly built windows.

Discrete outcomes (the chosen R1 / R2, the four front counts, det_flip, the gate's step, the status) must be identical; Rc, ric, the
singular values and the Huber weights must lie within 10x the restatement's own spread under a one-ulp perturbation of the points
(sfm_reference.perturb_ulp), as test_gpu_sfm.py does.  A fixture whose discrete outcome changes under that perturbation would not be a
fixture: the seeds below were chosen on the CPU so that none does, and fixture() asserts it.  The restatement of each window is
computed once and shared, and the step arrays are compared step by step, each against its own spread.

The windows carry 0.1 px of noise.  A noise-free pair is not a fixture: its essential matrix has two equal singular values, so the
order of v0 and v1, and with it det V and det_flip, changes under one ulp.

One thing in the reference's recursion is not determined by its inputs: after the first pair A has rank 2 (two equal smallest singular
values), so step 1's ric is any rotation of a one-parameter family, and the second pair's Huber weight, taken against that ric, is
anywhere in about [0.2, 1] at 8 or 15 degrees per frame (at 3 degrees the distance stays under the 5 degree knee).  That weight
stays in every later A.  The spread measures it, so those bars are wide where the result is arbitrary; test_recursion_without_huber
holds the same kernel tightly with the weighting switched off.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exrot_reference as xr  # noqa: E402

pytestmark = pytest.mark.gpu
PX = 1.0 / 460.0
PAIR_KEYS = ("n_corres", "front", "choice", "det_flip")
STEP_KEYS = ("step_q", "step_ric", "sigma", "huber", "q", "ric")


@pytest.fixture(scope="module")
def exrot_lib(vio, hip_lib):
    return vio.load_exrot()


def first_tracks(item, n):
    return dict(item, start_frame=item["start_frame"][:n], obs_offset=item["obs_offset"][:n + 1], pts=item["pts"][:item["obs_offset"][n]])


def build(name):
    if name == "deg8":
        return xr.make_window(1, 8, noise=0.1 * PX)[0]
    if name == "deg15":
        return xr.make_window(1, 15, noise=0.1 * PX)[0]
    if name == "deg3":
        return xr.make_window(1, 3, noise=0.1 * PX)[0]
    if name == "F2":                    # the smallest shape: a single pair, the gate never reachable
        return xr.make_window(4, 8, F=2, noise=0.1 * PX)[0]
    if name == "nine":
        return first_tracks(build("F2"), 9)
    if name == "eight":
        return first_tracks(build("F2"), 8)
    if name == "few":                   # fewer correspondences than a wavefront has lanes
        return first_tracks(build("F2"), 20)
    if name == "many":                  # more correspondences than the workgroup has threads
        return xr.make_window(6, 8, F=3, noise=0.1 * PX, n_points=2400)[0]
    if name == "no_tracks":
        return dict(n_frames=5, start_frame=np.zeros(0, dtype=np.int32), obs_offset=np.zeros(1, dtype=np.int64), pts=np.zeros((0, 2)),
                    delta_q=xr.make_window(1, 8, F=5, n_points=1)[0]["delta_q"])
    if name == "Fmax":
        return xr.make_window(5, 8, F=xr.MAX_FRAMES, noise=0.1 * PX, n_points=200)[0]
    raise KeyError(name)


_fixtures = {}


def fixture(name):
    """(item, restatement, spread): computed once; the discrete outcomes must survive the perturbation."""
    if name not in _fixtures:
        item = build(name)
        ref = xr.exrot(item)
        rng = np.random.RandomState(7)
        runs = [xr.exrot(xr.perturb_ulp(item, rng)) for _ in range(2)]
        for p in runs:
            assert (p["status"], p["step"]) == (ref["status"], ref["step"]), name
            for k in PAIR_KEYS:
                assert np.array_equal(p["pairs"][k], ref["pairs"][k]), (name, k)
        sp = {k: np.max([np.nan_to_num(np.abs(p[k] - ref[k])) for p in runs], axis=0) for k in STEP_KEYS}
        sp["Rc"] = np.max([np.nan_to_num(np.abs(p["pairs"]["Rc"] - ref["pairs"]["Rc"])) for p in runs], axis=0)
        _fixtures[name] = (item, ref, sp)
    return _fixtures[name]


def _close(got, ref, spread, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    m = ~np.isnan(ref)
    if not m.any():
        return
    bar = 10.0 * float(np.max(spread)) + 1e-13 * max(1.0, float(np.abs(ref[m]).max()))
    err = np.abs(got[m] - ref[m]).max()
    print("%-28s err %.3e  bar %.3e" % (what, err, bar))
    assert err <= bar, "%s: %.3e > %.3e" % (what, err, bar)


def check(name, g, ref, sp, ric=True):
    """ric=False: a window whose every A is rank-deficient by construction (a single pair, or every Rc the identity, where A^T A is a
    multiple of the identity): x is any vector of a plane or of the whole space, so ric is only held to being a rotation."""
    assert (g["status"], g["step"]) == (ref["status"], ref["step"]), (name, g["status"], g["step"], ref["status"], ref["step"])
    assert g["pairs"]["status"] == ref["pairs"]["status"], name
    for k in PAIR_KEYS:
        assert np.array_equal(g["pairs"][k], ref["pairs"][k]), (name, k, g["pairs"][k], ref["pairs"][k])
    _close(g["pairs"]["Rc"], ref["pairs"]["Rc"], sp["Rc"], name + ".Rc")
    for k in ("step_q", "step_ric", "sigma", "huber") if ric else ("sigma", "huber"):
        for i in range(len(ref[k])):
            _close(g[k][i], ref[k][i], sp[k][i], "%s.%s[%d]" % (name, k, i))
    for k in ("q", "ric"):
        _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))
    R = g["step_ric"]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() <= 1e-13 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-13, name
    assert np.abs(np.linalg.norm(g["step_q"], axis=1) - 1.0).max() <= 1e-13, name


def same(a, b):
    """Bitwise equality of two result dicts (NaN equal to NaN)."""
    for k in a:
        if k == "pairs":
            if not same(a[k], b[k]):
                return False
        elif not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"):
            return False
    return True


@pytest.mark.parametrize("name", ["deg8", "deg15", "deg3"])
def test_window_matches_restatement(exrot_lib, name):
    item, ref, sp = fixture(name)
    g = exrot_lib.create().exrot_batch([item])[0]
    check(name, g, ref, sp)
    if name == "deg3":
        assert g["status"] == xr.FAIL_NOT_OBSERVABLE and g["step"] == -1 and np.all(np.isfinite(g["step_ric"])) and np.all(np.isnan(g["ric"]))
    else:
        assert g["status"] == xr.OK and g["step"] == 10 and g["pairs"]["det_flip"].any()


@pytest.mark.parametrize("name", ["F2", "nine", "eight", "few", "many", "no_tracks", "Fmax"])
def test_shapes_at_the_limits(exrot_lib, name):
    item, ref, sp = fixture(name)
    g = exrot_lib.create().exrot_batch([item])[0]
    check(name, g, ref, sp, ric=name in ("many", "Fmax"))
    n = g["pairs"]["n_corres"]
    if name in ("F2", "nine", "eight", "few"):
        assert len(n) == 1 and g["status"] == xr.FAIL_NOT_OBSERVABLE        # one pair: the gate is never reachable
    if name == "nine":
        assert n[0] == 9 and g["pairs"]["choice"][0] in (1, 2)
    if name == "eight":
        assert n[0] == 8 and g["pairs"]["choice"][0] == 0 and np.array_equal(g["pairs"]["Rc"][0], np.eye(3))
    if name == "few":
        assert 9 <= n[0] < 64
    if name == "many":
        assert n.max() > 256
    if name == "no_tracks":
        assert np.all(n == 0) and np.array_equal(g["pairs"]["Rc"], np.stack([np.eye(3)] * 4))
    if name == "Fmax":
        assert len(n) == xr.MAX_FRAMES - 1 and g["status"] == xr.OK and g["step"] == 10


def test_other_gates(exrot_lib):
    """min_frames above F - 1 fails although sigma passes; a lower gate passes earlier; the steps are the same bits either way."""
    item, ref, sp = fixture("deg8")
    h = exrot_lib.create()
    full = h.exrot_batch([item])[0]
    h.set_config(min_frames=11)
    late = h.exrot_batch([item])[0]
    assert late["status"] == xr.FAIL_NOT_OBSERVABLE and late["step"] == -1 and late["sigma"][9][1] > 0.25
    h.set_config(min_frames=1, min_sigma=0.1)
    early = h.exrot_batch([item])[0]
    want = xr.calibrate(ref["pairs"]["Rc"], item["delta_q"], dict(min_frames=1, min_sigma=0.1))
    assert early["status"] == xr.OK and early["step"] == want["step"] and 1 < early["step"] < 10
    for r in (late, early):
        assert np.array_equal(r["step_ric"], full["step_ric"]) and np.array_equal(r["sigma"], full["sigma"])
    assert np.array_equal(early["ric"], full["step_ric"][early["step"] - 1])
    with pytest.raises(Exception, match="min_frames"):
        h.set_config(min_frames=0)


def test_recursion_without_huber(exrot_lib):
    """calibrate_batch from the restatement's own Rc with the weighting off (huber_deg far above every distance): from step 3 on the
    4 x 4 problem has rank 3 and every result is determined.  The bar is 10x the spread of the restatement over the perturbed runs' Rc."""
    h = exrot_lib.create()
    h.set_config(huber_deg=1e3)
    for name in ("deg8", "deg15"):
        item, ref, sp = fixture(name)
        rng = np.random.RandomState(3)
        want = xr.calibrate(ref["pairs"]["Rc"], item["delta_q"], dict(huber_deg=1e3))
        runs = [xr.calibrate(xr.exrot(xr.perturb_ulp(dict(item, n_frames=4), rng))["pairs"]["Rc"].tolist() + list(ref["pairs"]["Rc"][3:]),
                             item["delta_q"], dict(huber_deg=1e3)) for _ in range(2)]
        g = h.calibrate_batch([item], [ref["pairs"]["Rc"]])[0]
        assert (g["status"], g["step"]) == (want["status"], want["step"]) == (xr.OK, 10) and np.all(g["huber"] == 1.0)
        for k in ("step_q", "step_ric", "sigma"):
            for i in range(2, 10):
                _close(g[k][i], want[k][i], np.max([np.abs(p[k][i] - want[k][i]) for p in runs], axis=0), "%s.%s[%d]" % (name, k, i))


def test_huber_weight_on_a_wrong_imu_rotation(exrot_lib):
    """A pair whose delta_q is 20 degrees off gets the weight 5 / angle with the angle within a degree of 20 (the ric of the step
    before is within a degree of the truth by then), the pairs after it keep the weight 1, and the gate still passes at step 10."""
    import sfm_reference as sr
    item, ref, sp = fixture("deg8")
    dq = item["delta_q"].copy()
    dq[6] = sr.rot_to_quat(sr.quat_to_rot(dq[6]) @ sr.exp_so3(np.array([0.0, np.radians(20.0), 0.0])))
    g = exrot_lib.create().calibrate_batch([dict(item, delta_q=dq)], [ref["pairs"]["Rc"]])[0]
    want = xr.calibrate(ref["pairs"]["Rc"], dq)
    assert g["status"] == want["status"] == xr.OK and g["step"] == want["step"] == 10
    assert 5.0 / 21.0 <= g["huber"][6] <= 5.0 / 19.0 and 5.0 / 21.0 <= want["huber"][6] <= 5.0 / 19.0
    assert np.all(g["huber"][7:] == 1.0) and np.all(g["huber"][2:6] == 1.0)


def test_refusals_write_nothing(exrot_lib):
    h = exrot_lib.create()
    item, ref, sp = fixture("deg8")
    good = h.exrot_batch([item])[0]
    long = xr.make_window(5, 8, F=xr.MAX_FRAMES + 1, n_points=20)[0]
    for bad, msg in ((long, "window 1: n_frames"), (dict(build("no_tracks"), n_frames=1, delta_q=np.zeros((0, 4))), "window 1: n_frames")):
        import ctypes as C
        from vio_amd import exrot
        pk = exrot._Packed([item, bad])
        pairs = (exrot.VioExrotPair * (pk.total + 1))()
        res = (exrot.VioExrotResult * 2)()
        steps = (exrot.VioExrotStep * (pk.total + 1))()
        for buf in (pairs, res, steps):
            C.memset(C.addressof(buf), 0x5A, C.sizeof(buf))
        before = [bytes(buf) for buf in (pairs, res, steps)]
        st = exrot_lib.fn["batch"](h.h, 2, C.addressof(pk.items), C.addressof(pairs), C.addressof(res), C.addressof(steps))
        assert st == -1 and msg in h.last_error(), (st, h.last_error())              # VIO_ERR_BAD_ARG
        assert [bytes(buf) for buf in (pairs, res, steps)] == before
    leaves = dict(item, start_frame=item["start_frame"].copy())
    leaves["start_frame"][3] = 10
    with pytest.raises(Exception, match="window 0: track 3"):
        h.exrot_batch([leaves])
    assert same(h.exrot_batch([item])[0], good)


def test_non_finite_window_in_a_batch(exrot_lib):
    h = exrot_lib.create()
    a, c = fixture("deg8")[0], fixture("deg15")[0]
    pts = fixture("deg3")[0]["pts"].copy()
    pts[11, 1] = np.inf
    out = h.exrot_batch([a, dict(fixture("deg3")[0], pts=pts), c])
    assert "window 1" in h.last_error()
    b = out[1]
    assert b["status"] == xr.NOT_FINITE and b["pairs"]["status"] == xr.NOT_FINITE and b["step"] == -1
    for k in STEP_KEYS:
        assert np.all(np.isnan(b[k])), k
    assert np.all(np.isnan(b["pairs"]["Rc"]))
    alone = h.exrot_batch([a])[0], h.exrot_batch([c])[0]
    assert same(out[0], alone[0]) and same(out[2], alone[1])
    dq = a["delta_q"].copy()
    dq[2, 0] = np.nan
    r = h.exrot_batch([dict(a, delta_q=dq)])[0]
    assert r["status"] == xr.NOT_FINITE and r["pairs"]["status"] == xr.OK and same(r["pairs"], alone[0]["pairs"])


def test_batch_properties_hold_bitwise(exrot_lib):
    """Each window alone equals the window inside a mixed batch, in either order; a repeated call gives the same bits; the two
    stages called separately equal the combined call."""
    h = exrot_lib.create()
    names = ["deg8", "F2", "many", "no_tracks", "deg3", "Fmax", "eight"]
    items = [fixture(n)[0] for n in names]
    alone = [h.exrot_batch([it])[0] for it in items]
    fwd, again, rev = h.exrot_batch(items), h.exrot_batch(items), h.exrot_batch(items[::-1])[::-1]
    for n, a, f, g, r in zip(names, alone, fwd, again, rev):
        assert same(a, f) and same(a, g) and same(a, r), n
    pairs = h.relative_rotations_batch(items)
    cal = h.calibrate_batch(items, [p["Rc"] for p in pairs])
    for n, a, p, c in zip(names, alone, pairs, cal):
        assert same(p, a["pairs"]), n
        assert same(c, {k: v for k, v in a.items() if k != "pairs"}), n
    t = h.timing()
    assert np.isnan(t["pairs_ms"]) and t["solve_ms"] >= 0 and t["total_ms"] > 0
    assert h.exrot_batch([]) == []


def test_callers_device_is_restored(exrot_lib):
    import torch
    before = torch.cuda.current_device()
    exrot_lib.create(device=0).exrot_batch([fixture("F2")[0]])
    assert torch.cuda.current_device() == before
