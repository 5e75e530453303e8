"""StreamDriver(initialize=dict(sfm=True, calibrate_ric=...)) on the GPU: the driver starts from the identity as the camera-IMU
rotation, calibrates it on the window's own tracks and pre-integrated rotations (include/vio_exrot.h), then runs the SfM and the
alignment with it.

The streams are test_gpu_sfm_stream.py's (0.1 px of pixel noise, 60 landmarks per frame, tracks of 10 frames), 16 frames long.  They
rotate too little between frames for the reference's gate of 0.25: the second-smallest singular value at step 10 of the first window
is 0.0205 (synthetic) and 0.0156 (MH_05), so the gate is set to 0.01.  Measured first on the CPU, with the oracle library as the
backend and the restatements through the `calibrate_ric=`, `sfm=` and `aligner=` hooks (tests/test_exrot_reference.py runs that
twin without a GPU):
                                   ric error      aligned APE (rmse)
  SyntheticStream(16, seed 3)      0.2848 deg     0.0006 m     bounds: 0.5696 deg (twice), 0.01 m as test_gpu_init_stream.py
  RealImuStream (MH_05, seed 7)    0.7625 deg     0.0014 m     bounds: 1.5250 deg (twice), 0.03 m as test_gpu_init_stream.py
so the APE bounds of test_gpu_init_stream.py hold as they are.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exrot_reference as xr  # noqa: E402
from test_exrot_reference import CPU_RIC_ERR, make_stream  # noqa: E402

pytestmark = pytest.mark.gpu
GATE = dict(min_sigma=0.01)


@pytest.mark.parametrize("which,bound", [("syn", 0.01), ("mh", 0.03)])
def test_calibrated_stream_runs_to_the_end(vio, hip_lib, which, bound):
    from vio_amd import stream as vs, synth
    d = vs.StreamDriver(hip_lib, make_stream(vs, which, 16), seed=2, initialize=dict(sfm=True, calibrate_ric=GATE))
    assert np.array_equal(d.ext[3:7], [0.0, 0.0, 0.0, 1.0]) and np.array_equal(d.ext[0:3], d.s.ext[0:3])
    tr = d.run()
    assert d.init_tries == 1 and d.init_frame == 10 and d.init_exrot_status == [0] and d.init_sfm_status == [0]
    assert d.init_result["status"] == 0 and len(tr) == 16 - 10
    r = d.init_exrot_result
    err = xr.rot_error_deg(r["ric"], synth.quat_to_rot(d.s.ext[3:7]))
    e = vs.ape_stats(tr, d.ground_truth())["rmse"]
    print("%s: sigma at step 10 %.4f, ric error %.4f deg (CPU pipeline %.4f), APE %.4f m" % (which, r["sigma"][9][1], err, CPU_RIC_ERR[which], e))
    assert r["step"] == 10 and r["sigma"][9][1] > 0.01
    assert err <= 2.0 * CPU_RIC_ERR[which], err
    assert e <= bound, e


def test_the_references_gate_fails_the_try(vio, hip_lib):
    """With the default gate of 0.25 the synthetic stream never calibrates: each try fails with TRY_FAILED_EXROT + 1 before the SfM is
    called, the window slides, and max_tries failures raise."""
    from vio_amd import exrot, stream as vs
    d = vs.StreamDriver(hip_lib, make_stream(vs, "syn", 16), seed=2, initialize=dict(sfm=True, calibrate_ric=True, max_tries=2))
    with pytest.raises(RuntimeError, match="last status %d" % (exrot.TRY_FAILED_EXROT + 1)):
        d.ensure_initialized()
    assert d.init_exrot_status == [1, 1] and d.init_sfm_status == [] and d.frames[0] == 1 and d._sfm_h is None


def test_initialize_batched_makes_one_calibration_call_per_group(vio, hip_lib):
    """Three synthetic drivers (one group) in batched rounds: the first round calibrates all three in one exrot_batch call, and each
    driver gets the rotation, tries, scale, poses and speed-biases it gets alone, bitwise."""
    from vio_amd import batch_stream, stream as vs
    cfg = dict(sfm=True, calibrate_ric=GATE)
    mk = lambda s: vs.SyntheticStream(n_frames=16, landmarks_per_frame=60, track_len=10, seed=s, pixel_noise=0.1 / 460.0)  # noqa: E731
    drivers = [vs.StreamDriver(hip_lib, mk(s), seed=2, initialize=cfg) for s in (3, 5, 6)]
    calls = []
    h = vio.load_exrot().create()
    h.set_config(**GATE)
    inner = h.exrot_batch
    h.exrot_batch = lambda items: (calls.append(len(items)), inner(items))[1]
    drivers[0]._exrot_h = h
    batch_stream.initialize_batched(drivers)
    assert calls[0] == 3 and len(calls) == max(d.init_tries for d in drivers)
    for s, d in zip((3, 5, 6), drivers):
        alone = vs.StreamDriver(hip_lib, mk(s), seed=2, initialize=cfg)
        alone.ensure_initialized()
        assert np.array_equal(alone.ext, d.ext) and alone.init_tries == d.init_tries and alone.init_result["s"] == d.init_result["s"]
        assert alone.init_exrot_status == d.init_exrot_status
        assert np.array_equal(alone.poses, d.poses) and np.array_equal(alone.sb, d.sb)


def test_without_calibrate_ric_nothing_changes(vio, hip_lib):
    """initialize=dict(sfm=True) without `calibrate_ric` keeps the stream's own rotation and never creates the library's handle."""
    from vio_amd import stream as vs
    a = vs.StreamDriver(hip_lib, make_stream(vs, "syn", 14), seed=2, initialize=dict(sfm=True))
    b = vs.StreamDriver(hip_lib, make_stream(vs, "syn", 14), seed=2, initialize=dict(sfm=True, calibrate_ric=None))
    assert np.array_equal(a.ext, a.s.ext)
    ta, tb = a.run(), b.run()
    assert a._exrot_h is None and b._exrot_h is None and not a.init_exrot_status and np.array_equal(ta, tb)
