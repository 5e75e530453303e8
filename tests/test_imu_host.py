"""The IMU pre-integration library's host side without a GPU: its exported surface, the CSR packing of the Python binding, and the
stream driver's default, which must not touch the library."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_imu_library_exports_its_header_and_nothing_else(vio):
    hdr = open(os.path.join(ROOT, "include", "vio_imu.h")).read()
    declared = set(re.findall(r"\b(vio_imu_\w+)\s*\(", hdr))
    assert {"vio_imu_create", "vio_imu_destroy", "vio_imu_last_error", "vio_imu_load", "vio_imu_propagate"} <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", vio.IMU_LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-2] in ("T", "W", "B", "D", "V")}
    ours = {n for n in exported if "vio" in n.lower() or n.startswith("k_")}
    assert ours == declared, (sorted(ours - declared), sorted(declared - ours))
    lib = vio.ImuLib(vio.IMU_LIB)
    assert lib.fn["version"]() == 1


def test_pack_intervals_is_the_csr_of_the_samples(vio):
    rng = np.random.RandomState(0)
    ivs = []
    for S in (3, 0, 1, 5):
        ivs.append(dict(acc0=rng.normal(size=3), gyr0=rng.normal(size=3), dt=list(rng.uniform(0, 1, S)),
                        acc=list(rng.normal(size=(S, 3))), gyr=list(rng.normal(size=(S, 3)))))
    off, first, dt, acc, gyr = vio.imu.pack_intervals(ivs)
    assert off.dtype == np.int64 and list(off) == [0, 3, 3, 4, 9]
    assert dt.shape == (9,) and acc.shape == (9, 3) and gyr.shape == (9, 3) and first.shape == (4, 6)
    for i, iv in enumerate(ivs):
        assert np.array_equal(first[i], np.concatenate([iv["acc0"], iv["gyr0"]]))
        sl = slice(off[i], off[i + 1])
        assert np.array_equal(dt[sl], np.asarray(iv["dt"]))
        assert np.array_equal(acc[sl], np.asarray(iv["acc"]).reshape(-1, 3))
        assert np.array_equal(gyr[sl], np.asarray(iv["gyr"]).reshape(-1, 3))
    off, first, dt, acc, gyr = vio.imu.pack_intervals([dict(acc0=np.zeros(3), gyr0=np.zeros(3), dt=[], acc=[], gyr=[])])
    assert list(off) == [0, 0] and dt.shape == (0,) and acc.shape == (0, 3)


def test_record_dict_round_trips_a_vio_preint(vio):
    rng = np.random.RandomState(1)
    iv = dict(acc0=rng.normal(size=3), gyr0=rng.normal(size=3), dt=[0.005] * 7, acc=list(rng.normal(size=(7, 3))),
              gyr=list(rng.normal(size=(7, 3))))
    d = vio.synth.preintegrate(iv["acc0"], iv["gyr0"], np.full(3, 0.1), np.full(3, 0.01), iv["dt"], iv["acc"], iv["gyr"])
    back = vio.imu.record_dict(vio.VioPreint.from_dict(d))
    assert set(back) == set(d)
    for k in d:
        assert np.array_equal(np.asarray(back[k]), np.asarray(d[k])), k


def test_the_default_driver_never_loads_the_imu_library(vio, oracle_lib, monkeypatch):
    def refuse():
        raise AssertionError("bias_relinearize=None loaded the IMU library")
    monkeypatch.setattr(vio, "load_imu", refuse)
    runs = []
    for kw in ({}, {"bias_relinearize": None}):
        st = vio.stream.SyntheticStream(n_frames=14, landmarks_per_frame=20, seed=3)
        drv = vio.stream.StreamDriver(oracle_lib, st, seed=1, nonkey_every=3, **kw)
        runs.append(drv.run())
        assert drv.repropagated == []
    assert np.array_equal(runs[0], runs[1])


# ---- what test_gpu_imu_limits.py rests on, without a GPU: the host routine (vio_preintegrate, no kernel) and the numpy restatement --
def test_host_routine_against_the_numpy_restatement(vio):
    """The measurement behind test_gpu_imu_limits.py's bound: the largest per-block relative difference between vio_preintegrate and
    vio.synth.preintegrate over imu_reference.limits_inputs().  Both run on the CPU and differ by rounding order alone; the value
    measured when the bound was set is imu_reference.HOST_VS_NUMPY, and the host routine, like the device, stays within
    NUMPY_FACTOR times it."""
    import imu_reference as ir
    hip = vio.load_hip()
    worst = (0.0, None)
    for name, ivs, ba, bg, noise in ir.limits_inputs(vio):
        if name == "ragged":
            assert sorted({len(iv["dt"]) for iv in ivs}) == list(ir.LIMIT_SIZES)
        for k, iv in enumerate(ivs):
            h, r = ir.host_record(hip, iv, ba[k], bg[k], noise), ir.numpy_record(vio, iv, ba[k], bg[k], noise)
            assert np.array_equal(ir.vec(h)[11:17], ir.vec(r)[11:17])
            d, blk = ir.worst_block(h, r)
            if d > worst[0]:
                worst = (d, (name, k, len(iv["dt"])) + blk)
    print("\nhost against numpy: largest block difference %.4e at %s (recorded: %.3e)" % (worst[0], worst[1], ir.HOST_VS_NUMPY))
    assert 0.0 < worst[0] <= ir.NUMPY_FACTOR * ir.HOST_VS_NUMPY, worst


def test_zero_dt_samples_on_the_host_and_in_numpy(vio):
    """The rule test_gpu_imu_limits.py asks of the device: the acc and gyr of a dt == 0 sample that no dt != 0 sample reads as a0 / g0
    change nothing, those of one that is read do."""
    import imu_reference as ir
    hip = vio.load_hip()
    ivs = ir.zero_dt_intervals()
    ba, bg = np.full(3, 0.05), np.full(3, -0.01)
    for record in (lambda iv: ir.host_record(hip, iv, ba, bg, ir.RAGGED_NOISE), lambda iv: ir.numpy_record(vio, iv, ba, bg, ir.RAGGED_NOISE)):
        base, same, other = [ir.vec(record(iv)).copy() for iv in ivs]
        assert np.array_equal(base, same)
        assert not np.array_equal(base[1:11], other[1:11]) and not np.array_equal(base[242:467], other[242:467])
