"""stream.step_group and stream.init_round: a StreamDriver alone is a group of one.  On the CPU oracle backend with the stand-in
handles (fm_outlier_reference.NumpyFmOutlier, est_init_reference.EstimatorInitReference, the numpy SfM and aligner), a driver run
through step() / ensure_initialized() and its twin run through batch_stream.step_batched([d], marg) / initialize_batched([d]) make
the same calls with the same arguments on their handles.  stream_group_util.OracleMarg marginalises each job through a fresh oracle
context's load + marginalize, the calls OwnContexts makes on the driver's own context, and the oracle's marginalisation is a function
of the loaded window alone: so here the two entry points agree in every bit, not only up to the first marginalisation."""
import inspect

import numpy as np

import est_init_reference as eir
import fm_outlier_reference as fo
import fm_stream_reference as fsr
import init_reference as ir
import sfm_reference as sr
from stream_group_util import ArgRecording, OracleMarg, patch_batched, stub_driver
from test_stream import same_stops

FM_SLOT, EST_SLOT = 3, 5


def same_calls(a, b):
    assert [c[0] for c in a.args] == [c[0] for c in b.args]
    for k, (x, y) in enumerate(zip(a.args, b.args)):
        assert x == y, (k, x[0])
    assert a.calls == b.calls


def same_tracks(a, b, slot):
    ta, tb = a.tracks_get(slot), b.tracks_get(slot)
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape and ta[k].tobytes() == tb[k].tobytes(), k


def same_state(a, b, slot):
    sa, sb = a.state_get(slot), b.state_get(slot)
    assert sorted(sa) == sorted(sb)
    for k in sa:
        va, vb = np.asarray(sa[k]), np.asarray(sb[k])
        assert va.shape == vb.shape and va.astype(np.float64).tobytes() == vb.astype(np.float64).tobytes(), k


def test_a_group_of_one_is_the_driver_alone(vio, oracle_lib, monkeypatch):
    """features= and state= on recording handles, outlier_px and nonkey_every=3 (both slide kinds) over a 16-frame stream: step() and
    step_batched([d], marg) give both handles the same (method, arguments), the records of the first frame byte for byte and the rest
    of the run inside tests/test_stream.py's bar between two implementations (positions within 1e-3 m, ATE within 1 %, same_stops)."""
    vs, bs = vio.stream, vio.batch_stream
    patch_batched(monkeypatch, oracle_lib)
    tri = oracle_lib.context().triangulate

    def make():
        fm, est = ArgRecording(fo.NumpyFmOutlier(tri)), ArgRecording(eir.EstimatorInitReference(vio.synth.preintegrate))
        d = stub_driver(vs.StreamDriver(oracle_lib, vs.SyntheticStream(n_frames=16, seed=2), triangulate=True, nonkey_every=3, outlier_px=3.0,
                                        features=(fm, FM_SLOT), state=(est, EST_SLOT)))
        d.ctx.get_stream = lambda: None                 # (the CPU backend has no stream to share)
        return d, fm, est
    (a, fm_a, est_a), (b, fm_b, est_b) = make(), make()
    while a.step():
        pass
    bs._check([b])
    marg = OracleMarg(oracle_lib)
    while bs.step_batched([b], marg)[0]:
        pass
    assert len(a.trajectory) == len(b.trajectory) == 6 and set(a.flags) == {vio.capi.MARG_OLD, vio.capi.MARG_SECOND_NEW}
    # the first frame, up to its marginalisation: the first window, the flags, the triangulated count, the keyframe decisions
    for k in fsr.WINDOW_FIELDS:
        assert fm_a.exports[FM_SLOT][0][k].tobytes() == fm_b.exports[FM_SLOT][0][k].tobytes(), k
    assert a.trajectory[0][0] == b.trajectory[0][0] and a.trajectory[0][1].tobytes() == b.trajectory[0][1].tobytes()
    assert a.flags == b.flags and a.n_triangulated == b.n_triangulated and a.fm_keyframe == b.fm_keyframe
    assert a.rejected == b.rejected and a.rejected_ids == b.rejected_ids and a.fm_erased == b.fm_erased and sum(a.rejected) > 10
    same_calls(fm_a, fm_b)
    same_calls(est_a, est_b)
    same_tracks(fm_a, fm_b, FM_SLOT)
    same_state(est_a, est_b, EST_SLOT)
    ta = np.array([np.concatenate([[t], p]) for t, p in a.trajectory])
    tb = np.array([np.concatenate([[t], p]) for t, p in b.trajectory])
    assert np.abs(ta[:, 1:4] - tb[:, 1:4]).max() < 1e-3
    gt = a.ground_truth()
    assert abs(vs.ate_rmse(ta, gt) - vs.ate_rmse(tb, gt)) <= 0.01 * vs.ate_rmse(ta, gt)
    same_stops(a.reports, b.reports)
    assert [f["failure"] for f in a.failures] == [f["failure"] for f in b.failures] == [0] * 6


def init_pair(vio, oracle_lib):
    """Two identical INITIAL drivers with sfm, an aligner whose first call fails, state= and features= on recording handles."""
    vs = vio.stream
    base = ir.make_aligner(oracle_lib)
    tri = oracle_lib.context().triangulate

    def make():
        n = []

        def aligner(items, intervals, tic, g_norm, noise):
            n.append(len(items))
            return [dict(status=1) for _ in items] if len(n) == 1 else base(items, intervals, tic, g_norm, noise)
        fm, est = ArgRecording(fsr.NumpyFm(tri)), ArgRecording(eir.EstimatorInitReference(vio.synth.preintegrate))
        st = vs.SyntheticStream(n_frames=14, landmarks_per_frame=60, track_len=10, seed=3, pixel_noise=0.1 / 460.0)
        d = vs.StreamDriver(oracle_lib, st, seed=2, triangulate=True, features=(fm, FM_SLOT),
                            initialize=dict(sfm=lambda items: [sr.sfm(it) for it in items], aligner=aligner, state=(est, EST_SLOT)))
        return d, fm, est
    return make(), make()


def test_a_round_of_one_is_the_driver_alone(vio, oracle_lib):
    """ensure_initialized() and initialize_batched([d]) over a failed first try: the same calls with the same arguments on the
    FeatureManager and the estimator-state handle, the same slots, and the same s, frames and depths."""
    (a, fm_a, est_a), (b, fm_b, est_b) = init_pair(vio, oracle_lib)
    a.ensure_initialized()
    assert vio.batch_stream.initialize_batched([b]) == 2
    assert a.initialized and b.initialized and a.init_tries == b.init_tries == 2 and a.init_frame == b.init_frame == 11
    same_calls(fm_a, fm_b)
    same_calls(est_a, est_b)
    names = [c[0] for c in est_a.calls]
    assert names[:22] == ["imu_batch", "image_batch"] * 11 and names[22:] == ["slide_batch", "imu_batch", "image_batch", "init_apply_batch"]
    assert [c[0] for c in fm_a.calls][11:] == ["tracks_batch", "slide_batch", "add_batch", "tracks_batch", "init_depth_batch"]
    same_tracks(fm_a, fm_b, FM_SLOT)
    same_state(est_a, est_b, EST_SLOT)
    assert float(a.init_result["s"]).hex() == float(b.init_result["s"]).hex() and a.frames == b.frames == list(range(1, 12))
    assert a.inv_depth.tobytes() == b.inv_depth.tobytes() and a.have_depth.sum() > 100


def test_no_parameter_says_the_caller_did_it(vio, oracle_lib):
    """No function of the two modules and no StreamDriver method takes fm_done, fm_batched, est_batched or observe, and a failed try
    leaves no _fm_gone behind: what left the window is init_apply's return value."""
    vs, bs = vio.stream, vio.batch_stream
    gone = {"fm_done", "fm_batched", "est_batched", "observe"}
    fns = [f for mod in (vs, bs) for _, f in inspect.getmembers(mod, inspect.isfunction) if f.__module__ == mod.__name__]
    fns += [f for cls in (vs.StreamDriver, vs.OwnContexts, bs.BatchedCalls) for _, f in inspect.getmembers(cls, inspect.isfunction)]
    assert len(fns) > 60
    for f in fns:
        assert not gone & set(inspect.signature(f).parameters), f.__qualname__
    for name in ("init_apply", "slide_lists", "propagate_next_frame", "slide_mats", "init_round", "step_group"):
        assert any(f.__name__ == name for f in fns), name
    (a, _, _), (b, _, _) = init_pair(vio, oracle_lib)
    assert bs.initialize_batched([a, b]) == 2 and a.init_tries == b.init_tries == 2
    for d in (a, b):
        assert not hasattr(d, "_fm_gone") and "_fm_gone" not in vars(d)
    assert list(inspect.signature(vs.StreamDriver.init_apply).parameters) == ["self", "res"]
