"""libvio_exrot_hip.so (include/vio_exrot.h) at its limits, against the numpy restatement (tests/exrot_reference.py) on the windows of
tests/exrot_limits_inputs.py.  tests/test_exrot_limits_inputs_cpu.py proves on the CPU that each window is the fixture it claims to be.

The comparison is test_gpu_exrot.py's: discrete outcomes (status, step, n_corres, front, choice, det_flip, the NaN pattern) equal;
floating values within 10x the restatement's own spread under one-ulp perturbations of its inputs plus 1e-13 max(1, |ref|)
(test_gpu_exrot._close, which prints `err .. bar ..`).  Stage 1 perturbs the points, the stage-2 windows every entry of Rc and delta_q;
three perturbations each, the restatement computed once per window (xl.stage1, xl.stage2).

  A  k_exrot_pairs at the edges of its track partition (255 .. 4096 tracks in one pair, runs of threads without a correspondence,
     correspondences at the ends of a run, the strided loops at 63 .. 257 correspondences)
  B  pairs of 0, 8, 9 and more than 60 correspondences in one window, in both orders
  C  finite points whose fit is not finite
  D  k_exrot_solve alone: every branch of rot_to_quat, Huber weights that the inputs determine, the knee, the gate's edge, F = 2 and
     F = 32, 96 windows in one call
  E  refusals, a caller's stream, buffers that grow and are reused

The windows with ric at 2.8 rad do not recover ric: the quaternions of rotations beyond 120 degrees lose their sign consistency in the
reference's formulation and the smallest singular value ends near 2.4, not 0.  That is the reference's behaviour; the device is held to
the restatement there, not to the ground truth.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exrot_limits_inputs as xl  # noqa: E402
import exrot_reference as xr  # noqa: E402
from test_gpu_exrot import _close, check, same  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG = -1


@pytest.fixture(scope="module")
def exrot_lib(vio, hip_lib):
    return vio.load_exrot()


@pytest.fixture(scope="module")
def handle(exrot_lib):
    """One handle with the default configuration, shared by the tests that do not change it."""
    return exrot_lib.create()


def rotations(g, name):
    R = g["step_ric"]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() <= 1e-13 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-13, name
    assert np.abs(np.linalg.norm(g["step_q"], axis=1) - 1.0).max() <= 1e-13, name


def check_stage2(name, g, fx, ref=None, sp=None):
    """A stage-2 window against its restatement: from the first determined step on every value, before it (the 4 x 4 problem is
    rank-deficient by construction there) rotations only; the Huber weights at every step."""
    ref, sp, first = ref or fx["ref"], sp or fx["sp"], fx["first"]
    assert (g["status"], g["step"]) == (ref["status"], ref["step"]), (name, g["status"], g["step"], ref["status"], ref["step"])
    worst = 0.0
    for k in ("step_q", "step_ric", "sigma"):
        for i in range(first, len(ref[k])):
            _close(g[k][i], ref[k][i], sp[k][i], "%s.%s[%d]" % (name, k, i))
            worst = max(worst, np.abs(g[k][i] - ref[k][i]).max())
    _close(g["huber"], ref["huber"], sp["huber"], name + ".huber")
    for k in ("q", "ric"):
        _close(g[k], ref[k], sp[k], "%s.%s" % (name, k))
    rotations(g, name)
    print("%-10s largest device-to-restatement difference from step %d on: %.3e" % (name, first + 1, worst))


def raw_call(lib, h, fn, items, steps=True, rc=None, pairs=True, res=True):
    """The C entry point itself: (status, pairs, res, steps, packed) with ctypes arrays (None where not asked for)."""
    from vio_amd import exrot
    pk = exrot._Packed(items, tracks=rc is None)
    P = (exrot.VioExrotPair * (pk.total + 1))() if pairs and rc is None else None
    R = (exrot.VioExrotResult * len(items))() if res else None
    S = (exrot.VioExrotStep * (pk.total + 1))() if steps else None
    for buf in (P, R, S):
        if buf is not None:
            C.memset(C.addressof(buf), 0x5A, C.sizeof(buf))
    adr = lambda b: C.addressof(b) if b is not None else None       # noqa: E731
    if rc is not None:
        st = lib.fn[fn](h.h, len(items), C.addressof(pk.items), rc.ctypes.data, adr(R), adr(S))
    elif fn == "relative_rotations_batch":
        st = lib.fn[fn](h.h, len(items), C.addressof(pk.items), adr(P))
    else:
        st = lib.fn[fn](h.h, len(items), C.addressof(pk.items), adr(P), adr(R), adr(S))
    return st, P, R, S, pk


# ---- A: the partition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", xl.CUT_SIZES)
def test_cut_at_a_partition_edge(handle, n):
    """The first n tracks of one F = 2 window: C = ceil(n / 256) steps at 257 and 513, the last threads own nothing there, 4096 is
    VIO_EXROT_MAX_TRACKS; 63 .. 65 and 256, 257 correspondences are the edges of the `k += 256` and `e < 4 n` loops."""
    name = "cut%d" % n
    item, ref, sp = xl.stage1(name)
    g = handle.exrot_batch([item])[0]
    check(name, g, ref, sp, ric=False)
    assert g["pairs"]["n_corres"][0] == n and g["pairs"]["front"][0].max() == n
    if n == 4096:
        assert g["pairs"]["front"][0].tolist() == [0, 0, 4096, 0] and g["pairs"]["choice"][0] == 2


@pytest.mark.parametrize("name", ["sparse513", "sparse4096", "ends"])
def test_runs_without_a_correspondence(handle, name):
    """Whole runs of threads with mine == 0; a pair's correspondences at the first and the last track of a run (sparse), or all in
    the last run, all in the first, all between (ends)."""
    item, ref, sp = xl.stage1(name)
    g = handle.exrot_batch([item])[0]
    check(name, g, ref, sp)
    assert g["pairs"]["n_corres"].tolist() == {"sparse513": [114, 456], "sparse4096": [32, 4080], "ends": [16, 16, 4064]}[name]


# ---- B: unequal pairs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counts", [("unequal", xl.UNEQUAL), ("unequal_rev", xl.UNEQUAL[::-1])])
def test_thin_pairs_between_full_ones(handle, name, counts):
    """Pairs of 0, 8 and 9 correspondences among full ones: the identity enters the recursion between solved pairs, and every pair's
    scratch starts where the unequal ones before it end; the reversed order of sizes moves every offset."""
    item, ref, sp = xl.stage1(name)
    g = handle.exrot_batch([item])[0]
    check(name, g, ref, sp)
    for k, c in enumerate(counts):
        if c in (0, 8):
            assert g["pairs"]["n_corres"][k] == c and g["pairs"]["choice"][k] == 0 and np.array_equal(g["pairs"]["Rc"][k], np.eye(3))
            assert not g["pairs"]["front"][k].any()
        else:
            assert g["pairs"]["choice"][k] in (1, 2) and g["pairs"]["front"][k].max() == g["pairs"]["n_corres"][k]


# ---- C: finite points, a fit that is not finite --------------------------------------------------------------
def test_finite_points_with_a_fit_that_is_not_finite(exrot_lib, handle):
    """Every frame-0 point of pair 0 at one exactly representable point: the points are finite, so the kernel passes its first
    check, and the fit is not.  The pair keeps its n_corres, its Rc is NaN, and stage 2 of the same call turns the window NaN."""
    base, item = xl.degenerate_base(), xl.degenerate()
    left, right = xl.stage1("unequal")[0], xl.stage1("sparse513")[0]
    good = handle.exrot_batch([base])[0]
    alone = handle.exrot_batch([left])[0], handle.exrot_batch([right])[0]
    st, P, R, S, pk = raw_call(exrot_lib, handle, "batch", [left, item, right])
    assert st == xr.NOT_FINITE and "window 1" in handle.last_error(), (st, handle.last_error())
    lo, hi = int(pk.base[1]), int(pk.base[2])
    p0 = P[lo]
    assert p0.status == xr.NOT_FINITE and p0.n_corres == good["pairs"]["n_corres"][0] >= xr.MIN_CORRES
    assert np.all(np.isnan(p0.Rc[:])) and p0.front[:] == [0, 0, 0, 0] and p0.choice == 0 and p0.det_flip == 0
    for k in range(1, hi - lo):                                                      # frame 0 belongs to pair 0 only
        p = P[lo + k]
        assert p.status == xr.OK and p.n_corres == good["pairs"]["n_corres"][k] and p.front[:] == good["pairs"]["front"][k].tolist()
        assert p.choice == good["pairs"]["choice"][k] and bool(p.det_flip) == bool(good["pairs"]["det_flip"][k])
        assert np.array_equal(np.array(p.Rc[:]).reshape(3, 3), good["pairs"]["Rc"][k])
    assert R[1].status == xr.NOT_FINITE and R[1].step == -1 and np.all(np.isnan(R[1].q[:])) and np.all(np.isnan(R[1].R[:]))
    for k in range(lo, hi):
        assert np.all(np.isnan(S[k].q[:] + S[k].R[:] + S[k].sigma[:] + [S[k].huber])), k
    assert R[0].status == alone[0]["status"] and R[2].status == alone[1]["status"]
    out = handle.exrot_batch([left, item, right])
    assert same(out[0], alone[0]) and same(out[2], alone[1])
    pairs = handle.relative_rotations_batch([item])[0]
    assert "window 0" in handle.last_error() and same(pairs, out[1]["pairs"]) and pairs["status"] == xr.NOT_FINITE


# ---- D: stage 2 alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4))
def test_every_quaternion_branch(exrot_lib, i):
    """Rotations of 130 .. 176.5 degrees about axes near x, y and z with ric at 2.8 rad (i < 3) or 0.6 rad: Quaternion(Rc),
    Quaternion(Rimu) and Quaternion(Rc_g) take each of the three largest-diagonal branches (the table is in
    tests/test_exrot_limits_inputs_cpu.py).  Weighting off; from step 3 on every result is determined."""
    name = "branches%d" % i
    fx = xl.stage2(name)
    h = exrot_lib.create()
    h.set_config(**xl.NO_HUBER)
    g = h.calibrate_batch([fx["item"]], [fx["Rc"]])[0]
    assert (g["status"], g["step"]) == (xr.OK, 10) and np.all(g["huber"] == 1.0)
    check_stage2(name, g, fx)
    tab = xl.branch_table(fx["Rc"], fx["item"]["delta_q"], g)[0]                     # the device's own ric makes the same decisions
    assert np.array_equal(tab[fx["determined"]], fx["table"][fx["determined"]])


def test_determined_huber_weights(handle):
    """Weighting on, weights between 0.04 and 1 that the inputs determine; all four quaternion branches inside one window, and
    Quaternion(ric) off the trace branch."""
    fx = xl.stage2("huber")
    g = handle.calibrate_batch([fx["item"]], [fx["Rc"]])[0]
    check_stage2("huber", g, fx)
    assert np.array_equal(g["huber"] == 1.0, fx["ref"]["huber"] == 1.0) and (g["huber"] < 1.0).sum() >= 3
    tab = xl.branch_table(fx["Rc"], fx["item"]["delta_q"], g)[0]
    assert np.array_equal(tab[fx["determined"]], fx["table"][fx["determined"]])


def test_the_knee(handle):
    """A pair 4.9 degrees off keeps the weight 1 exactly, one 5.1 degrees off gets huber_deg / distance."""
    fx = xl.stage2("knee")
    g = handle.calibrate_batch([fx["item"]], [fx["Rc"]])[0]
    check_stage2("knee", g, fx)
    lo, hi = [k for k, v in xl.KNEE_PAIRS.items() if v[1] == 4.9][0], [k for k, v in xl.KNEE_PAIRS.items() if v[1] == 5.1][0]
    assert g["huber"][lo] == 1.0 and 0.9 < g["huber"][hi] < 1.0 and np.all(np.delete(g["huber"], hi) == 1.0)
    _close(g["huber"][hi], fx["ref"]["huber"][hi], fx["sp"]["huber"][hi], "knee.huber[%d]" % hi)


def test_gate_at_its_edge(exrot_lib):
    """sig[1] > min_sigma is strict: with min_sigma at the device's own sigma of the passing step the gate does not pass there, one
    ulp below it does; the steps are the same bits whatever the gate."""
    fx = xl.stage2("huber")
    item, Rc = fx["item"], fx["Rc"]
    h = exrot_lib.create()
    full = h.calibrate_batch([item], [Rc])[0]
    k = full["step"]
    v = float(full["sigma"][k - 1][1])
    assert full["status"] == xr.OK and k == 10 and v > xr.DEFAULT_CFG["min_sigma"]
    h.set_config(min_sigma=v)
    at = h.calibrate_batch([item], [Rc])[0]
    later = [j + 1 for j in range(len(Rc)) if j + 1 >= 10 and full["sigma"][j][1] > v]
    assert k not in later
    assert (at["status"], at["step"]) == ((xr.OK, later[0]) if later else (xr.FAIL_NOT_OBSERVABLE, -1)), (at["status"], at["step"], later)
    if later:
        assert np.array_equal(at["ric"], full["step_ric"][later[0] - 1]) and np.array_equal(at["q"], full["step_q"][later[0] - 1])
    h.set_config(min_sigma=float(np.nextafter(v, 0.0)))
    below = h.calibrate_batch([item], [Rc])[0]
    assert (below["status"], below["step"]) == (xr.OK, k) and np.array_equal(below["ric"], full["ric"])
    for r in (at, below):
        for key in ("step_q", "step_ric", "sigma", "huber"):
            assert np.array_equal(r[key], full[key]), key
    print("gate: step %d at sigma %.17g; at that min_sigma step %d" % (k, v, at["step"]))
    # min_frames = 1: the first step whose sigma passes, on F = 17 and on a single pair (F = 2, where none can)
    h.set_config(min_frames=1)
    want = xr.calibrate(Rc, item["delta_q"], dict(min_frames=1))
    assert np.abs(want["sigma"][:, 1] - 0.25).min() > 1e-6 and 1 < want["step"] < 10
    early = h.calibrate_batch([item], [Rc])[0]
    assert (early["status"], early["step"]) == (xr.OK, want["step"]) and np.array_equal(early["step_ric"], full["step_ric"])
    one = h.calibrate_batch([dict(n_frames=2, delta_q=item["delta_q"][3:4])], [Rc[3:4]])[0]
    want = xr.calibrate(Rc[3:4], item["delta_q"][3:4], dict(min_frames=1))
    assert (one["status"], one["step"]) == (want["status"], want["step"]) == (xr.FAIL_NOT_OBSERVABLE, -1) and np.all(np.isnan(one["ric"]))
    # min_frames = 32 on F = 32: 31 steps never reach it
    fb = xl.stage2("branches3")
    h.set_config(min_frames=32, **xl.NO_HUBER)
    never = h.calibrate_batch([fb["item"]], [fb["Rc"]])[0]
    h.set_config(**xl.NO_HUBER)
    usual = h.calibrate_batch([fb["item"]], [fb["Rc"]])[0]
    assert (never["status"], never["step"]) == (xr.FAIL_NOT_OBSERVABLE, -1) and np.all(np.isnan(never["ric"])) and usual["step"] == 10
    assert never["sigma"][30][1] > 0.25 and all(np.array_equal(never[key], usual[key]) for key in ("step_q", "step_ric", "sigma", "huber"))


def test_single_pair_through_stage_two(handle):
    """F = 2 through calibrate_batch alone.  One pair leaves A with rank 2: sigma[0] and the weight are determined and held to the
    standard bar; the two smaller singular values are square roots of rounding residues of a zero eigenvalue (about 1e-8 at most
    whichever side computes them), so they are held to being that small, and ric to being a rotation."""
    fx = xl.stage2("huber")
    item, Rc = dict(n_frames=2, delta_q=fx["item"]["delta_q"][3:4]), fx["Rc"][3:4]   # 20 degrees, against the identity: weight 0.51
    ref = xr.calibrate(Rc, item["delta_q"])
    rng = np.random.RandomState(7)
    runs = [xr.calibrate(Rc2, it2["delta_q"]) for it2, Rc2 in (xl.perturb_stage2(item, Rc, rng) for _ in range(xl.N_PERTURB))]
    g = handle.calibrate_batch([item], [Rc])[0]
    assert (g["status"], g["step"]) == (ref["status"], ref["step"]) == (xr.FAIL_NOT_OBSERVABLE, -1)
    _close(g["sigma"][0][0], ref["sigma"][0][0], np.max([abs(p["sigma"][0][0] - ref["sigma"][0][0]) for p in runs]), "F2.sigma[0][0]")
    _close(g["huber"], ref["huber"], np.max([np.abs(p["huber"] - ref["huber"]) for p in runs]), "F2.huber")
    assert ref["huber"][0] < 1.0 and g["sigma"][0][1:].max() <= 1e-6 and ref["sigma"][0][1:].max() <= 1e-6 and ref["sigma"][0][0] > 0.1
    rotations(g, "F2")


def test_ninety_six_windows_in_one_call(exrot_lib, handle):
    """F cycling over 2, 3, 11, 17, 31, 32: every window of the batch is bitwise its solo result, in either order, and the flat steps
    array holds each window's steps at the sum of the (n_frames - 1) before it, with steps given and with steps = NULL."""
    batch = xl.stage2_batch()
    items, Rcs = [b[0] for b in batch], [b[1] for b in batch]
    alone = [handle.calibrate_batch([it], [Rc])[0] for it, Rc in batch]
    fwd = handle.calibrate_batch(items, Rcs)
    rev = handle.calibrate_batch(items[::-1], Rcs[::-1])[::-1]
    for i, (a, f, r) in enumerate(zip(alone, fwd, rev)):
        assert same(a, f) and same(a, r), i
    assert {a["status"] for a in alone} == {xr.OK, xr.FAIL_NOT_OBSERVABLE}
    rc = np.concatenate([Rc.reshape(-1, 9) for Rc in Rcs])
    st, _, R, S, pk = raw_call(exrot_lib, handle, "calibrate_batch", items, rc=rc)
    assert st == xr.OK and pk.total == 1440 == len(rc)
    for i, a in enumerate(alone):
        lo = sum(it["n_frames"] - 1 for it in items[:i])
        assert lo == pk.base[i]
        for k in range(items[i]["n_frames"] - 1):
            s = S[lo + k]
            assert np.array_equal(s.q[:], a["step_q"][k]) and np.array_equal(np.array(s.R[:]).reshape(3, 3), a["step_ric"][k]), (i, k)
            assert np.array_equal(s.sigma[:], a["sigma"][k]) and s.huber == a["huber"][k], (i, k)
        assert (R[i].status, R[i].step) == (a["status"], a["step"]) and np.array_equal(R[i].q[:], a["q"], equal_nan=True), i
    assert bytes(S)[C.sizeof(S) - C.sizeof(S[0]):] == b"\x5a" * C.sizeof(S[0])       # nothing past the last step
    st, _, R2, _, _ = raw_call(exrot_lib, handle, "calibrate_batch", items, rc=rc, steps=False)
    assert st == xr.OK and bytes(R2) == bytes(R)


# ---- E: refusals and the handle ------------------------------------------------------------------------------
def test_too_many_tracks_are_refused(exrot_lib):
    """VIO_EXROT_MAX_TRACKS + 1 tracks in window 1 of 2: VIO_ERR_BAD_ARG, no output byte touched, and the handle goes on."""
    h = exrot_lib.create()
    ok = xl.stage1("cut257")[0]
    before = h.exrot_batch([ok])[0]
    over = xl.cut(xl.MAX_TRACKS + 1)
    assert len(over["start_frame"]) == 4097
    for fn in ("batch", "relative_rotations_batch"):
        st, P, R, S, pk = raw_call(exrot_lib, h, fn, [ok, over])
        assert st == BAD_ARG and "window 1: n_tracks" in h.last_error(), (st, h.last_error())
        for buf in (P, R, S):
            assert bytes(buf) == b"\x5a" * C.sizeof(buf)
    assert same(h.exrot_batch([ok])[0], before)
    assert h.exrot_batch([xl.cut(xl.MAX_TRACKS)])[0]["pairs"]["n_corres"][0] == xl.MAX_TRACKS      # the limit itself is accepted


def test_a_callers_stream(exrot_lib, handle):
    import torch
    stream = torch.cuda.Stream()
    h = exrot_lib.create(stream=stream.cuda_stream)
    assert stream.cuda_stream != 0
    big, fx = xl.stage1("cut4096")[0], xl.stage2("huber")
    assert same(h.exrot_batch([big])[0], handle.exrot_batch([big])[0])
    assert same(h.calibrate_batch([fx["item"]], [fx["Rc"]])[0], handle.calibrate_batch([fx["item"]], [fx["Rc"]])[0])
    del h
    torch.cuda.synchronize()


def test_buffers_grow_and_are_reused(exrot_lib):
    """A large call, a one-pair call and the large call again on one handle: the third is the first bit for bit, the second what a
    fresh handle gives."""
    h = exrot_lib.create()
    large = [xl.stage1(n)[0] for n in ("unequal", "cut4096", "ends", "sparse513")]
    small = [xl.stage1("cut63")[0]]
    first = h.exrot_batch(large)
    middle = h.exrot_batch(small)
    third = h.exrot_batch(large)
    assert all(same(a, b) for a, b in zip(first, third))
    assert same(middle[0], exrot_lib.create().exrot_batch(small)[0])
    grown = h.exrot_batch(large + large[::-1])                                       # and past the first size
    assert all(same(a, b) for a, b in zip(first + first[::-1], grown))
