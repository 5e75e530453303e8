"""Batched IMU pre-integration on the GPU (csrc/libvio_imu_hip.so, include/vio_imu.h) against the host's vio_preintegrate, interval for
interval: the real MH_05 stretch, a ragged random batch in one launch, re-propagation, the records in a solve, the errors, and the
stream driver's bias_relinearize option."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

VEC_TOL = 1e-13          # delta_p / delta_q / delta_v / sum_dt, relative to the vector's largest entry
BLOCK_TOL = 1e-12        # jacobian / covariance, per 3 x 3 block, relative to the block's largest entry


@pytest.fixture(scope="module")
def mh05():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))


@pytest.fixture(scope="module")
def imu_lib(vio, hip_lib):
    return vio.load_imu()


def mh05_intervals(vio, mh05):
    meas = np.concatenate([np.asarray(mh05["imu_acc"]), np.asarray(mh05["imu_gyr"])], axis=1)
    noise = dict(acc_n=float(mh05["acc_n"]), gyr_n=float(mh05["gyr_n"]), acc_w=float(mh05["acc_w"]), gyr_w=float(mh05["gyr_w"]))
    ivs, _ = vio.stream.cut_imu_intervals(np.asarray(mh05["imu_t"], dtype=np.float64), meas, [float(t) for t in mh05["cam_t"]], noise)
    return ivs, noise


def host_record(hip_lib, iv, ba, bg, noise):
    return hip_lib.preintegrate(iv["acc0"], iv["gyr0"], ba, bg, np.asarray(iv["dt"], dtype=np.float64).reshape(-1),
                                np.asarray(iv["acc"], dtype=np.float64).reshape(-1, 3), np.asarray(iv["gyr"], dtype=np.float64).reshape(-1, 3),
                                noise["acc_n"], noise["gyr_n"], noise["acc_w"], noise["gyr_w"])


def vec(p):
    return np.frombuffer(p, dtype=np.float64)


def check_close(got, ref, where=""):
    g, r = vec(got), vec(ref)
    for name, a, b in (("sum_dt", 0, 1), ("delta_p", 1, 4), ("delta_q", 4, 8), ("delta_v", 8, 11)):
        scale = max(np.abs(r[a:b]).max(), 1e-300)
        err = np.abs(g[a:b] - r[a:b]).max() / scale
        assert err <= VEC_TOL, (where, name, err)
    assert np.array_equal(g[11:17], r[11:17]), where                 # linearized_ba / bg: the biases used
    for name, o in (("jacobian", 17), ("covariance", 242)):
        G, R = g[o:o + 225].reshape(15, 15), r[o:o + 225].reshape(15, 15)
        for bi in range(5):
            for bj in range(5):
                gb, rb = G[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3], R[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3]
                err = np.abs(gb - rb).max()
                assert err <= BLOCK_TOL * np.abs(rb).max(), (where, name, bi, bj, err, np.abs(rb).max())


def test_mh05_parity_with_the_host(vio, hip_lib, imu_lib, mh05):
    ivs, noise = mh05_intervals(vio, mh05)
    assert len(ivs) == 35
    h = imu_lib.create()
    h.load(ivs, noise)
    for ba, bg in ((np.zeros(3), np.zeros(3)), (np.full(3, 0.05), np.full(3, 0.01))):
        got = h.propagate(ba, bg)
        assert len(got) == len(ivs)
        for k, iv in enumerate(ivs):
            check_close(got[k], host_record(hip_lib, iv, ba, bg, noise), "interval %d, ba %g" % (k, ba[0]))
    t = h.timing()
    assert t["kernel_ms"] > 0 and t["total_ms"] >= t["kernel_ms"]


def ragged_batch(n=1000, seed=11):
    rng = np.random.RandomState(seed)
    sizes = [0, 1, 2, 17, 200, 2000]
    ivs = []
    for i in range(n):
        S = sizes[i % len(sizes)]
        dt = rng.uniform(0.0005, 0.01, S)
        acc = rng.normal(0.0, 3.0, (S, 3)) + np.array([0.0, 0.0, 9.81])
        gyr = rng.uniform(-10.0, 10.0, (S, 3))
        ivs.append(dict(acc0=rng.normal(0.0, 3.0, 3), gyr0=rng.uniform(-10.0, 10.0, 3), dt=list(dt), acc=list(acc), gyr=list(gyr)))
    ba, bg = rng.normal(0.0, 0.1, (n, 3)), rng.normal(0.0, 0.02, (n, 3))
    return ivs, ba, bg


def test_random_ragged_batch_in_one_launch(vio, hip_lib, imu_lib):
    ivs, ba, bg = ragged_batch()
    noise = dict(acc_n=0.08, gyr_n=0.004, acc_w=2.0e-4, gyr_w=2.0e-6)
    h = imu_lib.create()
    h.load(ivs, noise)
    got = h.propagate(ba, bg)
    for k, iv in enumerate(ivs):
        check_close(got[k], host_record(hip_lib, iv, ba[k], bg[k], noise), "interval %d (%d samples)" % (k, len(iv["dt"])))


def test_repropagation_is_a_fresh_propagation(vio, imu_lib):
    ivs, ba, bg = ragged_batch(60, seed=5)
    b1, b2 = (ba, bg), (ba + 0.03, bg - 0.004)
    h = imu_lib.create()
    h.load(ivs)
    r1 = [vec(p).copy() for p in h.propagate(*b1)]
    out = (vio.VioPreint * len(ivs))()
    h.propagate(*b2, out=out)
    fresh = imu_lib.create()
    fresh.load(ivs)
    r2 = [vec(p).copy() for p in fresh.propagate(*b2)]
    for k in range(len(ivs)):
        assert np.array_equal(vec(out[k]), r2[k]), k
        if len(ivs[k]["dt"]):
            assert not np.array_equal(r1[k], r2[k]), k
    again = [vec(p).copy() for p in h.propagate(*b2)]
    assert all(np.array_equal(a, b) for a, b in zip(again, r2))          # two identical calls: bitwise equal
    # a subset: the listed records become b1's, every other one stays as it was
    which = [0, 5, 17, 42, 59, 5]
    got = h.propagate(*b1, which=which, out=out)
    assert [vec(p).tobytes() for p in got] == [r1[k].tobytes() for k in which]
    for k in range(len(ivs)):
        assert np.array_equal(vec(out[k]), r1[k] if k in which else r2[k]), k


def synthetic_window_intervals(vio):
    """The raw samples make_window pre-integrates (t0 = 1, 10 Hz frames, 200 Hz IMU)."""
    s = vio.synth
    times = [1.0 + 0.1 * i for i in range(vio.NUM_FRAMES)]
    ivs = []
    for i in range(vio.WINDOW_SIZE):
        ms = [s.motion_model(times[i] + k * 0.005) for k in range(21)]
        ivs.append(dict(acc0=ms[0].acc, gyr0=ms[0].gyro, dt=[0.005] * 20, acc=[m.acc for m in ms[1:]], gyr=[m.gyro for m in ms[1:]]))
    return ivs


def test_gpu_records_solve_like_the_host_records(vio, hip_lib, imu_lib):
    ivs = synthetic_window_intervals(vio)
    noise = dict(acc_n=vio.synth.ACC_N, gyr_n=vio.synth.GYR_N, acc_w=vio.synth.ACC_W, gyr_w=vio.synth.GYR_W)
    rng = np.random.RandomState(3)
    ba, bg = rng.normal(0.0, 0.02, (10, 3)), rng.normal(0.0, 0.002, (10, 3))
    h = imu_lib.create()
    h.load(ivs, noise)
    gpu = h.propagate(ba, bg)
    host = [host_record(hip_lib, iv, ba[k], bg[k], noise) for k, iv in enumerate(ivs)]
    states = []
    for pres in (host, gpu):
        w = vio.synth.make_window(64, seed=7)
        w.speed_bias[:10, 3:6], w.speed_bias[:10, 6:9] = ba, bg
        w.preint = list(pres)
        c = hip_lib.context()
        c.load(w)
        rep = c.solve(10)
        assert rep.final_chi2 < rep.initial_chi2
        poses, sb, _ = c.get_window()
        states.append((poses, sb, c.get_landmarks()))
    for a, b in zip(states[0], states[1]):
        assert np.abs(a - b).max() <= 1e-9


def raw(imu_lib):
    fn = imu_lib.fn
    h = C.c_void_p()
    assert fn["create"](0, None, C.byref(h)) == 0
    return fn, h


def test_errors_and_edge_cases(vio, hip_lib, imu_lib):
    BAD, NOT_FINITE = -1, -3
    fn = imu_lib.fn
    assert fn["create"](0, None, None) == BAD
    assert fn["create"](-1, None, C.byref(C.c_void_p())) == BAD
    fn, h = raw(imu_lib)
    try:
        ba = np.zeros((3, 3))
        out = (vio.VioPreint * 3)()
        assert fn["propagate"](h, 3, None, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == BAD       # nothing loaded
        assert b"nothing loaded" in fn["last_error"](h)
        pack_intervals = vio.imu.pack_intervals
        nz = vio.imu.VioImuNoise(0.08, 0.004, 2e-4, 2e-6)
        ivs = [dict(acc0=np.ones(3), gyr0=np.zeros(3), dt=[0.005] * 4, acc=[np.ones(3)] * 4, gyr=[np.full(3, 0.1)] * 4),
               dict(acc0=np.ones(3), gyr0=np.zeros(3), dt=[], acc=[], gyr=[]),
               dict(acc0=np.ones(3), gyr0=np.zeros(3), dt=[0.005] * 3, acc=[np.ones(3)] * 3, gyr=[np.full(3, 0.1)] * 3)]
        off, first, dt, acc, gyr = pack_intervals(ivs)
        load = lambda n, o, f=first.ctypes.data, noise=C.byref(nz): fn["load"](h, n, o.ctypes.data, f, dt.ctypes.data, acc.ctypes.data,
                                                                                gyr.ctypes.data, noise)
        assert load(-1, off) == BAD
        assert load(3, off, f=None) == BAD
        assert load(3, off, noise=None) == BAD
        assert load(3, np.array([1, 4, 4, 7], dtype=np.int64)) == BAD               # offset[0] != 0
        assert load(3, np.array([0, 4, 3, 7], dtype=np.int64)) == BAD               # decreasing
        assert fn["load"](h, 3, off.ctypes.data, first.ctypes.data, None, None, None, C.byref(nz)) == BAD
        assert load(3, off) == 0
        sentinel = np.frombuffer(out, dtype=np.float64)
        sentinel[:] = 7.0
        w_bad = np.array([0, 3], dtype=np.int32)
        assert fn["propagate"](h, 2, w_bad.ctypes.data, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == BAD
        assert fn["propagate"](h, 2, None, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == BAD     # NULL which: count must be n
        assert fn["propagate"](h, -1, w_bad.ctypes.data, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == BAD
        assert fn["propagate"](h, 3, None, None, ba.ctypes.data, C.addressof(out)) == BAD
        assert fn["propagate"](h, 3, None, ba.ctypes.data, ba.ctypes.data, None) == BAD
        assert np.all(sentinel == 7.0)                                                     # nothing written
        assert fn["propagate"](h, 0, None, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == BAD     # count 0 with NULL: not n
        assert fn["propagate"](h, 0, w_bad.ctypes.data, None, None, None) == 0            # an empty list: nothing to do
        # the zero-sample interval is not an error: the identity record
        assert fn["propagate"](h, 3, None, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == 0
        z = out[1]
        assert z.sum_dt == 0.0 and list(z.delta_q) == [0, 0, 0, 1] and list(z.delta_p) == [0] * 3 and list(z.delta_v) == [0] * 3
        assert np.array_equal(np.array(z.jacobian[:]).reshape(15, 15), np.eye(15))
        assert not np.any(np.array(z.covariance[:]))
        # a NaN sample: non-finite outputs for its interval, VIO_ERR_NOT_FINITE naming it, the others as always
        acc2 = acc.copy()
        acc2[5, 1] = np.nan                                                             # sample 5: interval 2's second
        assert fn["load"](h, 3, off.ctypes.data, first.ctypes.data, dt.ctypes.data, acc2.ctypes.data, gyr.ctypes.data, C.byref(nz)) == 0
        assert fn["propagate"](h, 3, None, ba.ctypes.data, ba.ctypes.data, C.addressof(out)) == NOT_FINITE
        assert b"interval 2" in fn["last_error"](h)
        assert not np.all(np.isfinite(np.frombuffer(out[2], dtype=np.float64)))
        assert np.all(np.isfinite(np.frombuffer(out[0], dtype=np.float64)))
        hh = imu_lib.create()
        hh.load([ivs[0], ivs[1], dict(ivs[2], acc=list(acc2[4:7]))])
        with pytest.raises(vio.VioError, match="interval 2"):
            hh.propagate(np.zeros(3), np.zeros(3))
    finally:
        fn["destroy"](h)


def test_the_callers_device_is_left_as_it_was(vio, imu_lib):
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        cur = torch.cuda.current_device()
        h = imu_lib.create(device=0)
        h.load(synthetic_window_intervals(vio))
        h.propagate(np.zeros(3), np.zeros(3))
        assert torch.cuda.current_device() == cur
        return
    torch.cuda.set_device(1)
    h = imu_lib.create(device=0)
    h.load(synthetic_window_intervals(vio))
    h.propagate(np.zeros(3), np.zeros(3))
    assert torch.cuda.current_device() == 1
    torch.cuda.set_device(0)


def run_mh05(vio, lib, mh05, **kw):
    st = vio.stream.RealImuStream(mh05, landmarks_per_frame=30, seed=7)
    drv = vio.stream.StreamDriver(lib, st, seed=2, **kw)
    traj = drv.run()
    return drv, traj, drv.ground_truth()


def test_stream_with_bias_relinearization(vio, hip_lib, mh05):
    d0, t0, gt = run_mh05(vio, hip_lib, mh05)
    dn, tn, _ = run_mh05(vio, hip_lib, mh05, bias_relinearize=None)
    assert np.array_equal(t0, tn)                                        # the default: bitwise the old trajectory
    assert dn.repropagated == [] and not hasattr(dn, "imu_h")
    db, tb, _ = run_mh05(vio, hip_lib, mh05, bias_relinearize=(0.1, 0.01))
    dz, tz, _ = run_mh05(vio, hip_lib, mh05, bias_relinearize=(0.0, 0.0))       # every interval, every step
    ate = {k: vio.stream.ate_rmse(t, gt) for k, t in (("zero_bias", t0), ("relinearize_0.1_0.01", tb), ("relinearize_always", tz))}
    ape = {k: vio.stream.ape_stats(t, gt)["rmse"] for k, t in (("zero_bias", t0), ("relinearize_0.1_0.01", tb), ("relinearize_always", tz))}
    print("\nMH_05 stream ATE (unaligned RMSE, m): %s; SE(3)-aligned: %s; intervals re-propagated: %d (0.1/0.01), %d (always)"
          % (ate, ape, sum(db.repropagated), sum(dz.repropagated)))
    assert len(tb) == len(t0) == len(tz) == 36 - 10
    assert ape["relinearize_0.1_0.01"] < 0.02 and ape["relinearize_always"] < 0.02
    assert all(np.isfinite(list(ate.values())))
    assert sum(dz.repropagated) > 0
