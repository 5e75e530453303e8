"""StreamDriver(initialize=dict(sfm=True)) on the GPU: the window starts from the window's own feature tracks (SfM library, then the
alignment library) instead of ground-truth camera poses, runs to the end, and run_batched initialises eight drivers with one SfM
call and one alignment call per round.

The streams carry 0.1 px of pixel noise (the default 1 px is three times the RANSAC gate of 0.3 px, under which the reference's own
"more than 12 points in front" test usually fails), 60 landmarks per frame and tracks of 10 frames.  Measured first on the CPU, with
the oracle library as the backend, tests/sfm_reference.py through the `sfm=` hook and tests/init_reference.py through `aligner=`
(aligned APE, `ape_stats(align=True)`, rmse in m; both initialise at the first try):
  SyntheticStream(30, seed 3)      0.0004  (ground-truth start 0.0003)      bound 0.01, as test_gpu_init_stream.py
  RealImuStream (MH_05, seed 7)    0.0038  (ground-truth start 0.0004)      bound 0.03, as test_gpu_init_stream.py
so the bounds of test_gpu_init_stream.py hold as they are.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PX = 1.0 / 460.0


def mh05():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mh05_imu_stretch.npz")))


def make(vs, which, n_frames=30, seed=None):
    if which == "syn":
        return vs.SyntheticStream(n_frames=n_frames, landmarks_per_frame=60, track_len=10, seed=3 if seed is None else seed,
                                  pixel_noise=0.1 * PX)
    return vs.RealImuStream(mh05(), landmarks_per_frame=60, track_len=10, seed=7 if seed is None else seed, pixel_noise=0.1 * PX)


@pytest.mark.parametrize("which,bound", [("syn", 0.01), ("mh", 0.03)])
def test_sfm_initialised_stream_runs_to_the_end(vio, hip_lib, which, bound):
    from vio_amd import stream as vs
    d0 = vs.StreamDriver(hip_lib, make(vs, which), seed=2)
    e0 = vs.ape_stats(d0.run(), d0.ground_truth())["rmse"]
    d = vs.StreamDriver(hip_lib, make(vs, which), seed=2, initialize=dict(sfm=True))
    tr = d.run()
    assert d.init_tries == 1 and d.init_frame == 10 and d.init_result["status"] == 0 and d.init_sfm_status == [0]
    assert len(tr) == len(d0.trajectory)
    e = vs.ape_stats(tr, d.ground_truth())["rmse"]
    print(which, "APE", e, "ground-truth start", e0, "s", d.init_result["s"])
    assert e <= bound and e0 <= bound, (e, e0)


def test_run_batched_initialises_like_the_drivers_alone(vio, hip_lib):
    from vio_amd import batch_stream, stream as vs
    cfg = dict(sfm=True)
    first = vs.StreamDriver(hip_lib, make(vs, "syn", 16, 0), initialize=cfg)
    sh = first.ctx.get_stream()
    batched = [first] + [vs.StreamDriver(hip_lib, make(vs, "syn", 16, s), ctx_kwargs=dict(stream=sh), initialize=cfg) for s in range(1, 8)]
    trajs = batch_stream.run_batched(batched, vio.load_marg().create(stream=sh))
    for s, d, tr in zip(range(8), batched, trajs):
        alone = vs.StreamDriver(hip_lib, make(vs, "syn", 16, s), initialize=cfg)
        ta = alone.run()
        assert d.init_result["status"] == 0 and alone.init_result["status"] == 0
        assert d.init_tries == alone.init_tries and d.init_result["s"] == alone.init_result["s"]
        assert d.init_sfm_status == alone.init_sfm_status
        assert tr.shape == ta.shape
        assert np.abs(tr - ta).max() <= 2e-2            # the tolerance of test_gpu_marg_batch's run_batched test


def test_initialize_batched_gives_each_driver_what_it_gets_alone(vio, hip_lib):
    """Synthetic and MH_05 drivers in batched rounds: the same tries, scale, poses and speed-biases, bitwise."""
    from vio_amd import batch_stream, stream as vs
    kinds = ["syn", "mh", "syn", "mh"]
    seeds = [3, 7, 5, 9]
    drivers = [vs.StreamDriver(hip_lib, make(vs, k, 14, s), seed=2, initialize=dict(sfm=True)) for k, s in zip(kinds, seeds)]
    batch_stream.initialize_batched(drivers)
    for k, s, d in zip(kinds, seeds, drivers):
        alone = vs.StreamDriver(hip_lib, make(vs, k, 14, s), seed=2, initialize=dict(sfm=True))
        alone.ensure_initialized()
        assert alone.init_tries == d.init_tries and alone.init_result["s"] == d.init_result["s"]
        assert np.array_equal(alone.poses, d.poses) and np.array_equal(alone.sb, d.sb)


def test_without_sfm_the_initialisation_is_unchanged(vio, hip_lib):
    """initialize=dict(...) without `sfm` never loads the SfM library's handle and gives the stand-in's trajectory, call after call."""
    from vio_amd import stream as vs
    a = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=4), seed=2, initialize=dict(scale=3.7))
    b = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=14, seed=4), seed=2, initialize=dict(scale=3.7, sfm=None))
    ta, tb = a.run(), b.run()
    assert a._sfm_h is None and b._sfm_h is None and not a.init_sfm_status
    assert np.array_equal(ta, tb)


def test_without_sfm_the_trajectories_are_the_parents(vio, hip_lib):
    """initialize=dict(...) without `sfm` gives, bit for bit, the trajectories of the commit before the SfM library: one driver
    alone on a synthetic stream and two MH_05 drivers through run_batched.  tests/golden/init_stream_parent.npz was recorded on an
    MI355X with that commit's Python package (stream.py, batch_stream.py, init.py, ...) over the product, IMU, marginalisation and
    alignment libraries, whose sources this feature does not touch, with exactly the calls below."""
    from vio_amd import batch_stream, stream as vs
    gold = np.load(os.path.join(GOLDEN_DIR, "init_stream_parent.npz"))
    d = vs.StreamDriver(hip_lib, vs.SyntheticStream(n_frames=20, seed=3), seed=2,
                        initialize=dict(scale=3.7, rot_noise=1e-3, pos_noise=1e-3, seed=1))
    assert np.array_equal(d.run(), gold["syn"])
    first = vs.StreamDriver(hip_lib, vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=7, n_frames=16), seed=2, initialize=dict(scale=2.0))
    sh = first.ctx.get_stream()
    second = vs.StreamDriver(hip_lib, vs.RealImuStream(mh05(), landmarks_per_frame=30, seed=8, n_frames=16), seed=2,
                             ctx_kwargs=dict(stream=sh), initialize=dict(scale=2.0, rot_noise=1e-3, seed=4))
    trs = batch_stream.run_batched([first, second], vio.load_marg().create(stream=sh))
    assert np.array_equal(trs[0], gold["mh_batched_0"]) and np.array_equal(trs[1], gold["mh_batched_1"])
