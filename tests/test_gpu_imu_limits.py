"""Batched IMU pre-integration on the GPU (csrc/libvio_imu_hip.so) against a reference that does not share its operation order, on
properties that need no reference, and at the edges of its interface.

Rule 1, the independent reference.  test_gpu_imu.py compares the device with the host's vio_preintegrate, which is written in the
device's operation order.  Here it is compared with vio.synth.preintegrate, the numpy restatement of IntegrationBase, block by
block (imu_reference.block_diffs: sum_dt, delta_p, delta_q, delta_v and the 3 x 3 blocks of the Jacobian and the covariance, each
relative to the block's largest entry; the biases exactly).  Inputs (imu_reference.limits_inputs): a ragged random batch of 96
intervals of 0, 1, 2, 3, 4, 5, 17 and 200 samples (seed 23, test_gpu_imu.py's distributions and noise), and the 35 intervals of the
recorded MH_05 stretch at zero biases and at biases 0.05 / 0.01.  Bound: the host routine and the numpy restatement, both on the
CPU, differ on exactly these inputs by at most 7.982e-16 in any block (covariance block (1, 0) of a 200-sample interval; MH_05:
6.39e-16 and 6.21e-16) -- rounding order alone.  The device's MFMA sums are a third order whose rounding may stack on the other
two, so the device is held to 4 x 7.99e-16 = 3.2e-15 against numpy.  test_imu_host.py repeats the measurement without a GPU.

Rule 2, properties of every record of those inputs: the covariance symmetric to 1e-12 of its largest entry and its smallest
eigenvalue at least -1e-12 of the largest; | |delta_q| - 1 | at most 4 ulp; sum_dt the left-to-right sum of the interval's dt, bit
for bit; and the Jacobian's blocks that F's structure forces.  F (integration_base.h:118-133 as host_dense.cpp's preintegrate
restates it, state order p, theta, v, ba, bg) has unit rows for ba and bg, and its theta rows have entries in the theta and bg
columns only.  J = F_k ... F_1 therefore has rows 9..14 equal to the identity's, exactly: blocks (3, 3) and (4, 4) are I and
(3, 0..2), (3, 4), (4, 0..3) are 0; and of columns 9..14 the blocks (1, 3) (theta does not depend on ba), (4, 3) and (3, 4) are 0.
The other blocks of those columns -- (0, 3), (2, 3), (0, 4), (1, 4), (2, 4) -- are the bias Jacobians proper and are free.

Rule 3, samples with dt == 0 (the recurrence in vio_imu.hip, h = dt): every term a sample's own acc and gyr enter is multiplied by
h, so with h == 0 the state, J and C come out of the sample as they went in -- but a0 and g0 carry the sample's values into the
next one.  The acc and gyr of a dt == 0 sample can therefore not matter exactly when no sample with dt != 0 reads them as a0 / g0:
when the next sample has dt == 0 too, or when it is the interval's last.  Such values are replaced and the record must not change
by a bit; the values of a dt == 0 sample followed by a sample with dt != 0 do matter, and the control shows that they do.

Rules 4 and 5: `which` in descending order, of length 1 and listing every interval twice gives the full propagation's records bit
for bit; a second vio_imu_load of another size on the same handle (the device buffer is released and allocated again) leaves no
trace; n == 0 loads, propagates nothing, and refuses count = 1 without writing.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imu_reference as ir  # noqa: E402
import test_gpu_imu as tgi  # noqa: E402  (check_close and its tolerances)

pytestmark = pytest.mark.gpu

ULP = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def imu_lib(vio, hip_lib):
    return vio.load_imu()


@pytest.fixture(scope="module")
def inputs(vio):
    """limits_inputs() with the numpy restatement's records, computed once for the module."""
    return [(name, ivs, ba, bg, noise, [ir.numpy_record(vio, iv, ba[k], bg[k], noise) for k, iv in enumerate(ivs)])
            for name, ivs, ba, bg, noise in ir.limits_inputs(vio)]


@pytest.fixture(scope="module")
def device_records(imu_lib, inputs):
    out = []
    for name, ivs, ba, bg, noise, _ in inputs:
        h = imu_lib.create()
        h.load(ivs, noise)
        out.append([ir.vec(p).copy() for p in h.propagate(ba, bg)])
        h.close()
    return out


@pytest.mark.parametrize("which", [0, 1, 2], ids=["ragged", "mh05_zero_bias", "mh05_biased"])
def test_device_against_the_numpy_restatement(inputs, device_records, which):
    name, ivs, ba, bg, noise, ref = inputs[which]
    got = device_records[which]
    assert len(got) == len(ivs) == (96 if which == 0 else 35)
    bound = ir.NUMPY_FACTOR * ir.HOST_VS_NUMPY
    worst, by_size = (0.0, None), {}
    for k, iv in enumerate(ivs):
        assert np.array_equal(got[k][11:17], np.concatenate([ba[k], bg[k]])), k      # linearized_ba / bg: the biases used
        d, blk = ir.worst_block(got[k], ref[k])
        S = len(iv["dt"])
        by_size[S] = max(by_size.get(S, 0.0), d)
        if d > worst[0]:
            worst = (d, (k, S) + blk)
    print("\n%s: device against numpy, largest block difference %.3e at (interval, samples, block) %s; by samples %s; bound %.3e"
          % (name, worst[0], worst[1], {S: "%.2e" % v for S, v in sorted(by_size.items())}, bound))
    if which == 0:
        assert sorted(by_size) == list(ir.LIMIT_SIZES)
    assert worst[0] <= bound, worst


def test_properties_that_need_no_reference(inputs, device_records):
    I3, Z3 = np.eye(3), np.zeros((3, 3))
    for (name, ivs, _, _, _, _), recs in zip(inputs, device_records):
        for k, (iv, r) in enumerate(zip(ivs, recs)):
            where = (name, k, len(iv["dt"]))
            assert np.all(np.isfinite(r)), where
            Cv = r[242:467].reshape(15, 15)
            top = np.abs(Cv).max()
            assert np.abs(Cv - Cv.T).max() <= 1e-12 * top, where
            ev = np.linalg.eigvalsh(0.5 * (Cv + Cv.T))
            assert ev[0] >= -1e-12 * ev[-1], (where, ev[0], ev[-1])
            q = r[4:8].astype(np.longdouble)
            assert abs(float(np.sqrt(np.sum(q * q)) - 1)) <= 4 * ULP, where
            s = 0.0
            for h in iv["dt"]:
                s += float(h)
            assert r[0] == s, where
            J = r[17:242].reshape(15, 15)
            blk = lambda i, j: J[3 * i:3 * i + 3, 3 * j:3 * j + 3]
            for i in (3, 4):                                        # rows 9..14: the identity's
                for j in range(5):
                    assert np.array_equal(blk(i, j), I3 if i == j else Z3), (where, i, j)
            assert np.array_equal(blk(1, 3), Z3), where             # columns 9..14: theta does not depend on ba
            if not len(iv["dt"]):
                assert np.array_equal(J, np.eye(15)) and not Cv.any(), where


def test_samples_with_zero_dt(hip_lib, imu_lib):
    ivs = ir.zero_dt_intervals()
    rng = np.random.RandomState(32)
    ba, bg = rng.normal(0.0, 0.1, 3), rng.normal(0.0, 0.02, 3)
    h = imu_lib.create()
    h.load(ivs, ir.RAGGED_NOISE)
    got = h.propagate(ba, bg)
    for k, iv in enumerate(ivs):
        tgi.check_close(got[k], ir.host_record(hip_lib, iv, ba, bg, ir.RAGGED_NOISE), "zero-dt interval %d" % k)
    base, same, other = [ir.vec(p).copy() for p in got]
    assert np.array_equal(base, same)
    assert not np.array_equal(base[1:11], other[1:11]) and not np.array_equal(base[242:467], other[242:467])
    # the same interval without its last sample (dt == 0): that sample is an identity step, F = I and V = 0.  It leaves sum_dt,
    # delta_p, delta_v and J as they are, renormalises delta_q once more, and rounds the covariance once more (F C F^T is formed
    # from C's accumulator registers read as C^T, so the rounding asymmetry of C changes sides).
    cut = dict(ivs[0], dt=ivs[0]["dt"][:11], acc=ivs[0]["acc"][:11], gyr=ivs[0]["gyr"][:11])
    h.load([cut], ir.RAGGED_NOISE)
    short = h.propagate(ba, bg)[0]
    c = ir.vec(short).copy()
    assert np.array_equal(c[:4], base[:4]) and np.array_equal(c[8:242], base[8:242])
    assert np.abs(c[4:8] - base[4:8]).max() <= 2 * ULP
    tgi.check_close(short, got[0], "without the last zero-dt sample")


def test_which_in_any_order(vio, imu_lib):
    ivs, ba, bg = ir.ragged_batch(60, seed=5)
    n = len(ivs)
    h = imu_lib.create()
    h.load(ivs, ir.RAGGED_NOISE)
    full = [ir.vec(p).copy() for p in h.propagate(ba, bg)]
    for which in (list(range(n - 1, -1, -1)), [37], [n - 1], [k // 2 for k in range(2 * n)], list(range(n)) + list(range(n - 1, -1, -1))):
        out = (vio.VioPreint * n)()
        np.frombuffer(out, dtype=np.float64)[:] = 7.0
        got = h.propagate(ba, bg, which=which, out=out)
        assert len(got) == len(which)
        assert [ir.vec(p).tobytes() for p in got] == [full[k].tobytes() for k in which], which[:4]
        for k in range(n):                                          # the listed entries are written, no other
            assert np.array_equal(ir.vec(out[k]), full[k]) if k in which else np.all(ir.vec(out[k]) == 7.0), (which[:4], k)


def test_loading_another_size_on_the_same_handle(vio, imu_lib):
    big, ba, bg = ir.ragged_batch(60, seed=5)
    small, sba, sbg = ir.ragged_batch(3, seed=6, sizes=(17, 0, 5))
    h = imu_lib.create()
    h.load(big, ir.RAGGED_NOISE)
    first = [ir.vec(p).copy() for p in h.propagate(ba, bg)]
    h.load(small, ir.RAGGED_NOISE)
    mid = [ir.vec(p).copy() for p in h.propagate(sba, sbg)]
    h.load(big, ir.RAGGED_NOISE)
    last = [ir.vec(p).copy() for p in h.propagate(ba, bg)]
    assert len(first) == len(last) == 60 and all(np.array_equal(a, b) for a, b in zip(first, last))
    fresh = imu_lib.create()
    fresh.load(small, ir.RAGGED_NOISE)
    want = [ir.vec(p).copy() for p in fresh.propagate(sba, sbg)]
    assert len(mid) == 3 and all(np.array_equal(a, b) for a, b in zip(mid, want))
    # n == 0: loads, propagates nothing, and has no interval to list
    h.load([], ir.RAGGED_NOISE)
    assert h.propagate(np.zeros(3), np.zeros(3)) == []
    fn = imu_lib.fn
    assert fn["propagate"](h.h, 0, None, None, None, None) == 0
    out = (vio.VioPreint * 1)()
    sentinel = np.frombuffer(out, dtype=np.float64)
    sentinel[:] = 7.0
    b3, w0 = np.zeros((1, 3)), np.zeros(1, dtype=np.int32)
    assert fn["propagate"](h.h, 1, w0.ctypes.data, b3.ctypes.data, b3.ctypes.data, C.addressof(out)) == -1
    assert b"not an interval" in fn["last_error"](h.h)
    assert fn["propagate"](h.h, 1, None, b3.ctypes.data, b3.ctypes.data, C.addressof(out)) == -1
    assert np.all(sentinel == 7.0)
    h.load(small, ir.RAGGED_NOISE)                                  # ... and the handle still works
    again = [ir.vec(p).copy() for p in h.propagate(sba, sbg)]
    assert all(np.array_equal(a, b) for a, b in zip(again, want))
