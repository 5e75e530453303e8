"""Inputs and metric of test_gpu_imu_limits.py, shared with its CPU twin in test_imu_host.py: the intervals both are run on, the
independent numpy restatement of IntegrationBase (vio.synth.preintegrate) as records, and the per-block relative difference of two
records (the blocks test_gpu_imu.py's check_close compares: sum_dt, delta_p, delta_q, delta_v, and the 3 x 3 blocks of the Jacobian
and the covariance, each relative to the block's own largest entry)."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LIMIT_SIZES = (0, 1, 2, 3, 4, 5, 17, 200)
RAGGED_NOISE = dict(acc_n=0.08, gyr_n=0.004, acc_w=2.0e-4, gyr_w=2.0e-6)          # test_gpu_imu.py's

# The largest per-block relative difference between the host routine (vio_preintegrate, host_dense.cpp) and the numpy restatement
# over limits_inputs(), measured on the CPU: 7.982e-16, in covariance block (1, 0) of a 200-sample interval of the ragged batch
# (MH_05: 6.39e-16 at zero biases, 6.21e-16 at biases 0.05 / 0.01; by interval length 0: 0, 1: 3.5e-16, 2: 4.8e-16, 3: 3.5e-16,
# 4: 3.9e-16, 5: 3.3e-16, 17: 3.5e-16, 200: 8.0e-16).  test_imu_host.py measures it again and prints it.  The two differ by rounding
# order alone; the device's sums (MFMA accumulation) are a third order, whose rounding may stack on both: its bound against numpy
# is NUMPY_FACTOR times this.
HOST_VS_NUMPY = 7.99e-16
NUMPY_FACTOR = 4.0


def vec(p):
    return np.frombuffer(p, dtype=np.float64)


def ragged_batch(n, seed, sizes=LIMIT_SIZES):
    """test_gpu_imu.py's random ragged batch over other interval lengths: n intervals, interval i of sizes[i % len(sizes)] samples."""
    rng = np.random.RandomState(seed)
    ivs = []
    for i in range(n):
        S = sizes[i % len(sizes)]
        dt = rng.uniform(0.0005, 0.01, S)
        acc = rng.normal(0.0, 3.0, (S, 3)) + np.array([0.0, 0.0, 9.81])
        gyr = rng.uniform(-10.0, 10.0, (S, 3))
        ivs.append(dict(acc0=rng.normal(0.0, 3.0, 3), gyr0=rng.uniform(-10.0, 10.0, 3), dt=list(dt), acc=list(acc), gyr=list(gyr)))
    ba, bg = rng.normal(0.0, 0.1, (n, 3)), rng.normal(0.0, 0.02, (n, 3))
    return ivs, ba, bg


def mh05_intervals(vio):
    """The 35 camera-to-camera intervals of the recorded MH_05 stretch and its noise densities."""
    mh05 = dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))
    meas = np.concatenate([np.asarray(mh05["imu_acc"]), np.asarray(mh05["imu_gyr"])], axis=1)
    noise = dict(acc_n=float(mh05["acc_n"]), gyr_n=float(mh05["gyr_n"]), acc_w=float(mh05["acc_w"]), gyr_w=float(mh05["gyr_w"]))
    ivs, _ = vio.stream.cut_imu_intervals(np.asarray(mh05["imu_t"], dtype=np.float64), meas, [float(t) for t in mh05["cam_t"]], noise)
    return ivs, noise


def limits_inputs(vio):
    """[(name, intervals, ba (n, 3), bg (n, 3), noise)]: the ragged batch of LIMIT_SIZES (96 intervals, 12 of each length) and the
    MH_05 intervals at zero and at non-zero biases."""
    ivs, ba, bg = ragged_batch(96, seed=23)
    out = [("ragged", ivs, ba, bg, RAGGED_NOISE)]
    mh, noise = mh05_intervals(vio)
    n = len(mh)
    out.append(("mh05_zero_bias", mh, np.zeros((n, 3)), np.zeros((n, 3)), noise))
    out.append(("mh05_biased", mh, np.full((n, 3), 0.05), np.full((n, 3), 0.01), noise))
    return out


def _arrays(iv):
    return (np.asarray(iv["dt"], dtype=np.float64).reshape(-1), np.asarray(iv["acc"], dtype=np.float64).reshape(-1, 3),
            np.asarray(iv["gyr"], dtype=np.float64).reshape(-1, 3))


def host_record(hip_lib, iv, ba, bg, noise):
    """vio_preintegrate of the product library: the host routine, no GPU."""
    dt, acc, gyr = _arrays(iv)
    return hip_lib.preintegrate(iv["acc0"], iv["gyr0"], ba, bg, dt, acc, gyr, noise["acc_n"], noise["gyr_n"], noise["acc_w"], noise["gyr_w"])


def numpy_record(vio, iv, ba, bg, noise):
    """vio.synth.preintegrate as a VioPreint."""
    dt, acc, gyr = _arrays(iv)
    return vio.VioPreint.from_dict(vio.synth.preintegrate(iv["acc0"], iv["gyr0"], np.asarray(ba, dtype=np.float64),
                                                          np.asarray(bg, dtype=np.float64), dt, acc, gyr, **noise))


def block_diffs(got, ref):
    """{(name, i, j): |got - ref|_max / |ref|_max} over the blocks of two records; a block the reference has all zero is held to be
    zero (inf otherwise).  The biases (linearized_ba / bg) are not a block: they are compared exactly by the callers."""
    g, r = vec(got), vec(ref)
    out = {}

    def rel(a, b):
        d, s = np.abs(a - b).max(), np.abs(b).max()
        return 0.0 if d == 0.0 else (d / s if s > 0.0 else np.inf)

    for name, a, b in (("sum_dt", 0, 1), ("delta_p", 1, 4), ("delta_q", 4, 8), ("delta_v", 8, 11)):
        out[(name, 0, 0)] = rel(g[a:b], r[a:b])
    for name, o in (("jacobian", 17), ("covariance", 242)):
        G, R = g[o:o + 225].reshape(15, 15), r[o:o + 225].reshape(15, 15)
        for bi in range(5):
            for bj in range(5):
                out[(name, bi, bj)] = rel(G[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3], R[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3])
    return out


def worst_block(got, ref):
    """(difference, block) of the block of block_diffs() that differs most."""
    d = block_diffs(got, ref)
    k = max(d, key=d.get)
    return d[k], k


def zero_dt_intervals():
    """One interval three times: as it is, with the values that cannot matter replaced, and (the control) with values replaced that
    the next sample reads as a0 / g0.  dt == 0 at samples 4 and 5 (the middle) and 11 (the end) of 12."""
    rng = np.random.RandomState(31)
    S = 12
    dt = rng.uniform(0.002, 0.006, S)
    dt[[4, 5, 11]] = 0.0
    acc = rng.normal(0.0, 3.0, (S, 3)) + np.array([0.0, 0.0, 9.81])
    gyr = rng.uniform(-3.0, 3.0, (S, 3))
    base = dict(acc0=rng.normal(0.0, 3.0, 3), gyr0=rng.uniform(-3.0, 3.0, 3), dt=list(dt), acc=acc, gyr=gyr)
    same = dict(base, acc=acc.copy(), gyr=gyr.copy())
    for s in (4, 11):                                              # read by nobody: the next sample has dt == 0 / there is none
        same["acc"][s] = rng.normal(0.0, 30.0, 3)
        same["gyr"][s] = rng.uniform(-30.0, 30.0, 3)
    other = dict(base, acc=acc.copy(), gyr=gyr.copy())
    other["acc"][5] = acc[5] + 1.0                                 # sample 6 (dt != 0) starts from these
    other["gyr"][5] = gyr[5] + 0.5
    return [base, same, other]
