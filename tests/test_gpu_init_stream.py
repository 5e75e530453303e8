"""StreamDriver(initialize=...) on the GPU: the window starts from the alignment (include/vio_init.h) on the SfM stand-in instead of
ground truth, retries where the stand-in fails, runs to the end, and run_batched initialises eight drivers in batched rounds.

The APE bounds were measured first on the CPU, with the oracle library as the backend and tests/init_reference.py as the aligner
(aligned APE, `ape_stats(align=True)`, rmse in m):
  SyntheticStream(30, seed 3), noise-free stand-in at scale 3.7           0.0033  (ground-truth start 0.0018)
  ... 1 mrad / 1 mm of noise                                               0.0034
  RealImuStream (MH_05), noise-free stand-in at scale 3.7                 0.0093  (ground-truth start 0.0091)
  ... 1 mrad / 1 mm of noise (s = 2.28 for 3.7: the stretch starts near rest) 0.052
  ... 2 mrad / 10 mm, seed 0: the first try fails, the second succeeds
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mh05():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))


def ape(vs, d, tr):
    return vs.ape_stats(tr, d.ground_truth())["rmse"]


@pytest.mark.parametrize("which,cfg,bound", [
    ("syn", dict(scale=3.7), 0.01),
    ("syn", dict(scale=3.7, rot_noise=1e-3, pos_noise=1e-3, seed=1), 0.01),
    ("mh", dict(scale=3.7), 0.03),
    ("mh", dict(scale=3.7, rot_noise=1e-3, pos_noise=1e-3, seed=1), 0.15),
])
def test_initialised_stream_runs_to_the_end(vio, hip_lib, which, cfg, bound):
    from vio_amd import stream as vs
    mk = (lambda: vs.SyntheticStream(n_frames=30, seed=3)) if which == "syn" else (lambda: vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=7))
    d0 = vs.StreamDriver(hip_lib, mk(), seed=2)
    e0 = ape(vs, d0, d0.run())
    d = vs.StreamDriver(hip_lib, mk(), seed=2, initialize=cfg)
    tr = d.run()
    assert d.init_tries == 1 and d.init_frame == 10 and d.init_result["status"] == 0
    assert len(tr) == len(d0.trajectory)
    e = ape(vs, d, tr)
    assert e <= bound and e0 <= bound, (e, e0)
    if cfg.get("rot_noise", 0) == 0:
        assert abs(d.init_result["s"] / 3.7 - 1) <= 1e-3


def test_noisy_start_retries(vio, hip_lib):
    from vio_amd import stream as vs
    d = vs.StreamDriver(hip_lib, vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=7), seed=2,
                        initialize=dict(scale=1.0, rot_noise=2e-3, pos_noise=1e-2, seed=0, max_tries=20))
    tr = d.run()
    assert d.init_tries >= 2 and d.init_frame == 10 + d.init_tries - 1 and d.init_result["status"] == 0
    assert len(tr) == d.s.n_frames - d.init_frame and np.all(np.isfinite(tr))
    with pytest.raises(RuntimeError, match="no initialisation"):
        vs.StreamDriver(hip_lib, vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=7), seed=2,
                        initialize=dict(scale=1.0, rot_noise=2e-3, pos_noise=1e-2, seed=0, max_tries=1)).run()


def test_run_batched_initialises_like_the_drivers_alone(vio, hip_lib):
    from vio_amd import batch_stream, stream as vs
    cfgs = [dict(scale=3.7, rot_noise=1e-3, pos_noise=1e-3, seed=s) for s in range(8)]
    first = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=0), initialize=cfgs[0])
    sh = first.ctx.get_stream()
    batched = [first] + [vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=s), ctx_kwargs=dict(stream=sh), initialize=cfgs[s])
                         for s in range(1, 8)]
    trajs = batch_stream.run_batched(batched, vio.load_marg().create(stream=sh))
    for s, d, tr in zip(range(8), batched, trajs):
        alone = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=16, seed=s), initialize=cfgs[s])
        ta = alone.run()
        assert d.init_tries == alone.init_tries and d.init_result["s"] == alone.init_result["s"]
        assert tr.shape == ta.shape
        assert np.abs(tr - ta).max() <= 2e-2            # the tolerance of test_gpu_marg_batch's run_batched test


def test_default_driver_is_unchanged(vio, hip_lib):
    """initialize=None loads no library and leaves the trajectory bitwise as it was (the ground-truth start)."""
    from vio_amd import stream as vs
    a = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=4), seed=2)
    b = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=4), seed=2, initialize=None)
    assert b.initialized and b.init_frame is None
    ta, tb = a.run(), b.run()
    assert np.array_equal(ta, tb)
    assert np.array_equal(a.ground_truth(), b.ground_truth())


def test_initialize_batched_aligns_mixed_drivers_with_their_own_parameters(vio, hip_lib):
    """Synthetic and MH_05 drivers (different extrinsic, G and IMU noise) initialised in batched rounds get what each gets alone."""
    from vio_amd import batch_stream, stream as vs
    mk = [lambda: vs.SyntheticStream(n_frames=14, seed=3), lambda: vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=7)] * 2
    cfgs = [dict(scale=3.7), dict(scale=3.7), dict(scale=2.0, rot_noise=1e-3, seed=1), dict(scale=2.0, rot_noise=1e-3, seed=1)]
    drivers = [vs.StreamDriver(hip_lib, m(), seed=2, initialize=c) for m, c in zip(mk, cfgs)]
    batch_stream.initialize_batched(drivers)
    for m, c, d in zip(mk, cfgs, drivers):
        alone = vs.StreamDriver(hip_lib, m(), seed=2, initialize=c)
        alone.ensure_initialized()
        assert alone.init_tries == d.init_tries and alone.init_result["s"] == d.init_result["s"]
        assert np.array_equal(alone.poses, d.poses) and np.array_equal(alone.sb, d.sb)
