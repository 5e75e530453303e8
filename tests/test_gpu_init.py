"""The batched visual-inertial alignment on the GPU (include/vio_init.h) against the numpy restatement (tests/init_reference.py).

The normal matrices A * 1000 have condition numbers of 1e7 to 1e10 here, so a fixed tolerance would be a guess.  Every bar is 10x the
restatement's own spread when each of its inputs moves by one ulp (measured per window, in the test, over two such perturbations),
plus 1e-13 of the quantity's size for the entries whose spread happens to be zero.  Measured on the windows below (CPU): the spread of
s is 7e-15 to 3.2e-12 relative, of g 1.9e-14 to 4.8e-10 (F = 4), of x 8.7e-15 to 1.6e-10, of the poses 1.1e-15 to 5.8e-12.

The smallest windows (syn2, syn3: F = 2 and F = 3, systems 10 and 13 wide) have fewer equations (6 per interval) than unknowns: the
linear stage's matrix is singular and Eigen's LDLT returns what rounding leaves of the null space.  The restatement then fails the
gravity test, and the device must report the same status and the same NaN pattern; s_linear and g_linear, the only numbers such a
window returns, fall under the same spread rule (their spread is of order 1 to 10 there, so that is a weak statement; the status is
the strong one).  A window whose status a one-ulp perturbation changes could not be held to a status, so the frames were chosen on
the CPU among twelve starting frames each: frames 0-1 (|g_linear| = 4.6) and 3-5 (|g_linear| = 19.0) keep FAIL_GRAVITY under eight
one-ulp perturbations, where frames 0-2 (12.5, against G + 1 = 10.8) did not; the test asserts it for the two perturbations it makes.
syn5_two_keys is an F = 5 window whose is_key leaves two keyframes, the fewest the library accepts.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_reference as ir  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("s", "g", "g_world", "s_linear", "g_linear", "rot", "x", "poses", "speed_bias")


@pytest.fixture(scope="module")
def init_lib(vio, hip_lib):
    return vio.load_init()


def _item(vs, st, frames, scale=3.7, key=None, **kw):
    R, T = vs.visual_trajectory(st, frames, 0, scale, **kw)
    it = dict(R=R, T=T, pre=[st.preint[f] for f in frames[:-1]], is_key=key)
    return it


def windows(vio):
    """(name, item, tic, G): synthetic F = 11 with and without noise, F = 4 / 17 / 32 with keyframe flags, MH_05 with and without
    noise, and the two constructed failures."""
    from vio_amd import stream as vs
    syn = vs.SyntheticStream(n_frames=34, seed=0)
    mh = vs.RealImuStream(dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz"))))
    S = (vio.synth.T_IC, vio.synth.G_NORM)
    M = (mh.tic, mh.g_norm)
    out = [("syn11", _item(vs, syn, list(range(11))), *S),
           ("syn11_noisy", _item(vs, syn, list(range(5, 16)), rot_noise=1e-3, pos_noise=2e-3, seed=3), *S),
           ("syn4_keys", _item(vs, syn, list(range(4)), key=np.array([1, 0, 1, 1], bool)), *S),
           ("syn17_keys", _item(vs, syn, list(range(17)), key=np.arange(17) % 3 != 1), *S),
           ("syn32_keys", _item(vs, syn, list(range(32)), key=np.arange(32) % 4 != 2, rot_noise=5e-4, seed=1), *S),
           ("mh11", _item(vs, mh, list(range(11))), *M),
           ("mh11_noisy", _item(vs, mh, list(range(20, 31)), rot_noise=1e-3, pos_noise=1e-3, seed=5), *M)]
    for seed in range(4):        # MH_05's near-rest start: with noise some of these fail the linear stage's tests
        out.append(("mh_start_%d" % seed, _item(vs, mh, list(range(11)), scale=1.0, rot_noise=1e-3, pos_noise=3e-3, seed=seed), *M))
    neg = _item(vs, syn, list(range(11)))
    neg["T"] = -neg["T"]
    out.append(("neg_T", neg, *S))
    out.append(("g_off", _item(vs, syn, list(range(11))), S[0], S[1] + 3.0))
    # the smallest windows (the module's docstring): last, so that the windows above keep their places
    out += [("syn2", _item(vs, syn, [0, 1]), *S), ("syn3", _item(vs, syn, [3, 4, 5]), *S),
            ("syn5_two_keys", _item(vs, syn, list(range(5)), key=np.array([0, 1, 0, 0, 1], bool)), *S)]
    return out


SMALLEST = ("syn2", "syn3", "syn5_two_keys")


def _perturbed_spread(oracle_lib, item, tic, G, bg, ref, must_keep_status=False):
    rng = np.random.RandomState(11)
    spread = {k: np.zeros_like(np.asarray(ref[k], dtype=np.float64)) for k in FIELDS}
    for _ in range(2):
        p = ir.align(oracle_lib, ir.perturb_ulp(item, rng), tic, G, bg)
        if p["status"] != ref["status"]:
            assert not must_keep_status, "the restatement's status changes under one ulp: not a usable window"
            continue
        for k in FIELDS:
            d = np.abs(np.asarray(p[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64))
            spread[k] = np.fmax(spread[k], np.nan_to_num(d, nan=0.0))
    return spread


def _close(got, ref, spread, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    m = ~np.isnan(ref)
    if not m.any():
        return
    bar = 10.0 * np.max(spread) + 1e-13 * max(1.0, np.abs(ref[m]).max())
    err = np.abs(got[m] - ref[m]).max()
    assert err <= bar, "%s: %.3e > %.3e" % (what, err, bar)


def test_gyro_bias_matches_restatement(vio, oracle_lib, init_lib):
    ws = windows(vio)
    h = init_lib.create()
    bg = h.gyro_bias_batch([w[1] for w in ws])
    for (name, item, tic, G), b in zip(ws, bg):
        ref, st = ir.gyro_bias(oracle_lib, item, np.zeros(3))
        assert st == ir.OK
        rng = np.random.RandomState(2)
        spread = max(np.abs(ir.gyro_bias(oracle_lib, ir.perturb_ulp(item, rng), np.zeros(3))[0] - ref).max() for _ in range(2))
        assert np.abs(b - ref).max() <= 10 * spread + 1e-16, (name, b, ref, spread)


def test_align_matches_restatement(vio, oracle_lib, init_lib):
    ws = windows(vio)
    h = init_lib.create()
    bgs = np.array([ir.gyro_bias(oracle_lib, w[1], np.zeros(3))[0] for w in ws])
    # one call per (tic, G): the batch API takes one of each
    groups = {}
    for i, w in enumerate(ws):
        groups.setdefault((tuple(w[2]), w[3]), []).append(i)
    statuses = set()
    for (tic, G), idx in groups.items():
        got = h.align_batch([ws[i][1] for i in idx], np.array(tic), G, bgs[idx])
        for i, g in zip(idx, got):
            name, item = ws[i][0], ws[i][1]
            ref = ir.align(oracle_lib, item, np.array(tic), G, bgs[i])
            assert g["status"] == ref["status"], (name, g["status"], ref["status"])
            assert g["n_key"] == ref["n_key"]
            statuses.add(ref["status"])
            spread = _perturbed_spread(oracle_lib, item, np.array(tic), G, bgs[i], ref, must_keep_status=name in SMALLEST)
            for k in FIELDS:
                _close(g[k], ref[k], spread[k], "%s.%s" % (name, k))
            if name in SMALLEST:
                print(name, "status", ref["status"], "n_key", ref["n_key"], "s_linear", g["s_linear"], ref["s_linear"], "g_linear",
                      g["g_linear"], ref["g_linear"], "spread", float(np.max(spread["s_linear"])), float(np.max(spread["g_linear"])))
                if ref["status"] != ir.OK:             # the same NaN pattern, field by field (also part of _close)
                    for k in FIELDS:
                        assert np.array_equal(np.isnan(np.asarray(g[k], dtype=np.float64)), np.isnan(np.asarray(ref[k], dtype=np.float64))), (name, k)
    assert {ir.OK, ir.FAIL_SCALE, ir.FAIL_GRAVITY} <= statuses
    by_name = {w[0]: w[1] for w in ws}
    assert [len(by_name[k]["R"]) for k in SMALLEST] == [2, 3, 5] and int(np.sum(by_name["syn5_two_keys"]["is_key"])) == 2


def _batch_of(vio, n):
    ws = [w for w in windows(vio) if w[2] is not None and w[3] == vio.synth.G_NORM and w[0].startswith("syn")]
    items = [ws[k % len(ws)][1] for k in range(n)]
    return items


def _bits(outs):
    return [np.concatenate([np.atleast_1d(np.asarray(o[k], dtype=np.float64)).ravel() for k in FIELDS]).view(np.uint64) for o in outs]


def test_window_bits_alone_inside_256_and_repeated(vio, init_lib):
    h = init_lib.create()
    items = _batch_of(vio, 256)
    tic, G = vio.synth.T_IC, vio.synth.G_NORM
    bg = np.zeros((256, 3))
    bg[:, 2] = np.linspace(0, 1e-3, 256)
    big = _bits(h.align_batch(items, tic, G, bg))
    again = _bits(h.align_batch(items, tic, G, bg))
    assert all(np.array_equal(a, b) for a, b in zip(big, again))
    names = [w[0] for w in windows(vio) if w[3] == G and w[0].startswith("syn")]
    assert len(names) == 8 and [names[i % 8] for i in (250, 253, 254, 255)] == ["syn4_keys", "syn2", "syn3", "syn5_two_keys"]
    for i in (0, 37, 255, 250, 253, 254):       # the last four: F = 4 and the three smallest windows
        alone = _bits(h.align_batch([items[i]], tic, G, bg[i:i + 1]))[0]
        assert np.array_equal(alone, big[i]), i
    g1 = h.gyro_bias_batch(items)
    g2 = h.gyro_bias_batch(items)
    assert np.array_equal(g1.view(np.uint64), g2.view(np.uint64))
    for i in (37, 253, 254, 255):
        assert np.array_equal(h.gyro_bias_batch(items[i:i + 1]).view(np.uint64), g1[i:i + 1].view(np.uint64)), i


def test_argument_errors_write_nothing(vio, init_lib):
    from vio_amd.init import VioInitResult, _Packed
    h = init_lib.create()
    fn = init_lib.fn
    items = _batch_of(vio, 3)
    tic = np.ascontiguousarray(vio.synth.T_IC)
    bg = np.zeros((3, 3))

    def call(pk, count=3, res=None):
        res = (VioInitResult * 3)() if res is None else res
        for r in res:
            r.status, r.s = 77, 123.0
        x = np.full((3, 99), 5.0)
        st = fn["align_batch"](h.h, C.c_int32(count), C.addressof(pk.items) if pk else None, tic.ctypes.data, C.c_double(9.81),
                               bg.ctypes.data, C.addressof(res), x.ctypes.data, None, None)
        bo = np.full((3, 3), 5.0)
        st2 = fn["gyro_bias_batch"](h.h, C.c_int32(count), C.addressof(pk.items) if pk else None, bg.ctypes.data, bo.ctypes.data, None)
        assert all(r.status == 77 and r.s == 123.0 for r in res) and np.all(x == 5.0) and np.all(bo == 5.0)
        return st, st2

    pk = _Packed(items)
    pk.items[1].n_frames = 1
    assert call(pk) == (-1, -1)
    assert b"window 1" in fn["last_error"](h.h)
    pk = _Packed(items)
    pk.items[2].n_frames = 33
    assert call(pk) == (-1, -1)
    pk = _Packed(items)
    pk.items[0].R = None
    assert call(pk) == (-1, -1)
    pk = _Packed(items)
    assert call(pk, count=-1) == (-1, -1)
    assert call(None, count=2) == (-1, -1)
    key = np.zeros(11, dtype=np.uint8)
    key[3] = 1
    pk = _Packed(items)
    pk.items[0].is_key = key.ctypes.data               # one keyframe only
    assert call(pk)[0] == -1
    assert h.align_batch([], tic, 9.81, np.zeros((0, 3))) == []
    assert fn["align_batch"](h.h, 0, None, None, C.c_double(9.81), None, None, None, None, None) == 0


def test_nan_window_is_isolated(vio, init_lib):
    h = init_lib.create()
    items = _batch_of(vio, 5)
    tic, G = vio.synth.T_IC, vio.synth.G_NORM
    clean = h.align_batch(items, tic, G, np.zeros(3))
    bad = [dict(it) for it in items]
    bad[2]["T"] = np.array(bad[2]["T"], dtype=np.float64)
    bad[2]["T"][1, 0] = np.nan
    got = h.align_batch(bad, tic, G, np.zeros(3))
    assert got[2]["status"] == ir.NOT_FINITE and np.isnan(got[2]["s"]) and np.all(np.isnan(got[2]["poses"]))
    for i in (0, 1, 3, 4):
        assert got[i]["status"] == ir.OK
        assert np.array_equal(_bits([got[i]])[0], _bits([clean[i]])[0])
    bg, st = h.gyro_bias_batch([dict(items[0], R=np.full((11, 3, 3), np.nan))] + items[1:], status=True)
    assert st[0] == ir.NOT_FINITE and np.all(np.isnan(bg[0])) and np.all(st[1:] == ir.OK)
    with pytest.raises(vio.VioError):
        h.gyro_bias_batch([dict(items[0], R=np.full((11, 3, 3), np.nan))])


def test_initialize_batch_runs_the_whole_alignment(vio, oracle_lib, init_lib):
    """gyro -> re-propagation of every interval at (0, bg) -> align, against the restatement on the same re-propagated records."""
    from vio_amd import stream as vs
    st = vs.SyntheticStream(n_frames=14, seed=2)
    b = np.array([0.01, -0.02, 0.005])
    ivs = [dict(iv, gyr0=np.asarray(iv["gyr0"]) + b, gyr=[np.asarray(g) + b for g in iv["gyr"]]) for iv in st.imu[:10]]
    pre = [vio.synth.preintegrate(iv["acc0"], iv["gyr0"], np.zeros(3), np.zeros(3), iv["dt"], iv["acc"], iv["gyr"]) for iv in ivs]
    R, T = vs.visual_trajectory(st, list(range(11)), 0, 2.5)
    item = dict(R=R, T=T, pre=pre)
    h = init_lib.create()
    out = h.initialize_batch([item, item], [ivs, ivs], vio.load_imu().create(), vio.synth.T_IC, vio.synth.G_NORM)
    assert out[0]["status"] == ir.OK and np.abs(out[0]["bg"] - b).max() <= 2e-4
    assert abs(out[0]["s"] / 2.5 - 1) <= 1e-3
    assert np.all(out[0]["speed_bias"][:, 6:9] == out[0]["bg"])
    assert all(np.array_equal(np.asarray(p["linearized_bg"]), out[0]["bg"]) for p in out[0]["pre"])
    ref = ir.align(oracle_lib, dict(item, pre=out[0]["pre"]), vio.synth.T_IC, vio.synth.G_NORM, out[0]["bg"])
    spread = _perturbed_spread(oracle_lib, dict(item, pre=out[0]["pre"]), vio.synth.T_IC, vio.synth.G_NORM, out[0]["bg"], ref)
    for k in FIELDS:
        _close(out[0][k], ref[k], spread[k], k)
    assert np.array_equal(_bits(out[:1])[0], _bits(out[1:])[0])


def test_the_callers_device_is_left_as_it_was(vio, init_lib):
    import torch
    items = _batch_of(vio, 2)
    if torch.cuda.device_count() < 2:
        cur = torch.cuda.current_device()
        h = init_lib.create(device=0)
        h.align_batch(items, vio.synth.T_IC, vio.synth.G_NORM, np.zeros(3))
        h.gyro_bias_batch(items)
        assert torch.cuda.current_device() == cur
        return
    torch.cuda.set_device(1)
    h = init_lib.create(device=0)
    h.align_batch(items, vio.synth.T_IC, vio.synth.G_NORM, np.zeros(3))
    h.gyro_bias_batch(items)
    assert torch.cuda.current_device() == 1
    torch.cuda.set_device(0)


def test_device_takes_the_quirk_branches(vio, oracle_lib, init_lib):
    """The constructed windows of tests/init_reference.py on the device: gravity exactly on +z (TangentBasis's exact comparison),
    exactly on -z (its degenerate basis, FromTwoVectors' antiparallel branch with an exactly opposite vector), 0.9 above G (the
    refined-scale failure), and MH_05 seen from a frame whose z points against gravity (the antiparallel branch's Householder QR on a
    vector 1e-11 off the axis).  Each agrees with the restatement as the other windows do, its status included."""
    from vio_amd import stream as vs
    tic = np.array([0.05, 0.04, 0.03])
    cases = [("up", ir.vertical_window(down=False)[0], tic, 9.81), ("down", ir.vertical_window(down=True)[0], tic, 9.81),
             ("heavy", ir.vertical_window(g_true=9.81 + 0.9)[0], tic, 9.81)]
    mh = vs.RealImuStream(dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz"))))
    item = _item(vs, mh, list(range(11)))
    g_true = (mh.R[0] @ mh.ric).T @ np.array([0.0, 0.0, mh.g_norm])
    cases.append(("mh_minus_z", ir.rotate_window(item, ir.rotation_onto(g_true / np.linalg.norm(g_true), [0.0, 0.0, -1.0])),
                  mh.tic, mh.g_norm))
    h = init_lib.create()
    want = {"up": ir.OK, "down": ir.OK, "heavy": ir.FAIL_REFINED_SCALE, "mh_minus_z": ir.OK}
    for name, it, t, G in cases:
        ref = ir.align(oracle_lib, it, t, G, np.zeros(3))
        got = h.align_batch([it], t, G, np.zeros(3))[0]
        assert ref["status"] == want[name] and got["status"] == ref["status"], (name, got["status"], ref["status"])
        if name != "heavy":
            assert ir.from_two_vectors_z(ir.normalized(list(got["g"])))[1] == (name != "up")
            assert np.abs(got["g_world"] - [0, 0, G]).max() <= 1e-9 * G
        spread = _perturbed_spread(oracle_lib, it, t, G, np.zeros(3), ref)
        for k in FIELDS:
            _close(got[k], ref[k], spread[k], "%s.%s" % (name, k))
    got = h.align_batch([cases[0][1]], tic, 9.81, np.zeros(3))[0]
    assert list(got["g_linear"][:2]) == [0.0, 0.0] and list(got["g"][:2]) == [0.0, 0.0]     # a == (0,0,1) exactly on the device too


def test_non_finite_gyro_step_clears_the_window(vio, init_lib):
    """initialize_batch: a window whose gyro step is not finite is VIO_ERR_NOT_FINITE with every output NaN, the others unaffected."""
    from vio_amd import stream as vs
    st = vs.SyntheticStream(n_frames=14, seed=2)
    R, T = vs.visual_trajectory(st, list(range(11)), 0, 2.5)
    good = dict(R=R, T=T, pre=st.preint[:10])
    bad = dict(good, R=np.array(R))
    bad["R"][3, 0, 0] = np.nan
    h = init_lib.create()
    out = h.initialize_batch([good, bad], [st.imu[:10]] * 2, vio.load_imu().create(), vio.synth.T_IC, vio.synth.G_NORM)
    assert out[0]["status"] == ir.OK and out[1]["status"] == ir.NOT_FINITE
    for k in FIELDS:
        assert np.all(np.isnan(np.asarray(out[1][k], dtype=np.float64))), k
