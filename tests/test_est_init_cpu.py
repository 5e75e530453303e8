"""The stream drivers on an estimator-state slot from the first IMU sample (initialize=dict(state=)) and with bias-following
pre-integrations in the slot (state=dict(relinearize=)), on the CPU: the oracle backend, tests/est_init_reference.py's stand-in handle,
the numpy aligner of tests/init_reference.py, and synth.preintegrate behind ImuHandle's two methods where a comparator needs the IMU
library."""
import numpy as np
import pytest

import est_init_reference as eir
import est_reference as er
import fm_stream_reference as fsr
import init_reference as ir


class NumpyImu:
    """ImuLib and ImuHandle for bias_relinearize= without a GPU: load + propagate over synth.preintegrate."""

    def __init__(self, vio):
        self.vio, self.ivs, self.noise, self.created = vio, [], {}, 0

    def create(self, device=0, stream=None):
        self.created += 1
        return self

    def load(self, intervals, noise=None):
        self.ivs, self.noise = [dict(iv) for iv in intervals], dict(noise or {})

    def propagate(self, ba, bg, which=None):
        n = len(self.ivs)
        ba, bg = np.broadcast_to(np.asarray(ba, dtype=np.float64), (n, 3)), np.broadcast_to(np.asarray(bg, dtype=np.float64), (n, 3))
        out = []
        for i in (range(n) if which is None else which):
            iv = self.ivs[i]
            out.append(self.vio.capi.VioPreint.from_dict(self.vio.synth.preintegrate(iv["acc0"], iv["gyr0"], ba[i].copy(), bg[i].copy(), list(iv["dt"]),
                                                                                     list(iv["acc"]), list(iv["gyr"]), **self.noise)))
        return out


@pytest.fixture
def numpy_imu(vio, monkeypatch):
    imu = NumpyImu(vio)
    monkeypatch.setattr(vio, "load_imu", lambda: imu)
    return imu


def stream16(vio):
    return vio.stream.SyntheticStream(n_frames=16, seed=3)


def failing_first(oracle_lib, fail_first):
    base, n = ir.make_aligner(oracle_lib), dict(n=0)

    def aligner(items, intervals, tic, g_norm, noise):
        n["n"] += 1
        if fail_first and n["n"] == 1:
            return [dict(status=1) for _ in items]
        return base(items, intervals, tic, g_norm, noise)
    return aligner


def fed_state(vio, st, ext, g_norm, failed):
    """The slot as the reference's processIMU / processImage / slideWindow leave it in the INITIAL state after `failed` failed tries,
    straight from the stream: one sample in front of the first image, eleven frames, then per failed try a slide and a frame."""
    s = er.new_state(tic=ext[0:3], ric=ext[3:7], g=(0.0, 0.0, g_norm))
    s, _ = er.process_imu(s, [0.0], [st.imu[0]["acc0"]], [st.imu[0]["gyr0"]])
    s = er.process_image(s, st.times[0], True)
    for k in range(1, 11 + failed):
        if k > 10:
            s, slid, _ = er.slide_window(s, er.MARG_OLD)
            assert slid == 1
        iv = st.imu[k - 1]
        s, status = er.process_imu(s, iv["dt"], iv["acc"], iv["gyr"])
        assert status == 0
        s = er.process_image(s, st.times[k], True)
    return s


def same_state(a, b):
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert va.shape == vb.shape and va.astype(np.float64).tobytes() == vb.astype(np.float64).tobytes(), k


@pytest.mark.parametrize("fail_first", [False, True])
def test_a_stream_lives_in_its_slot_from_the_first_sample(vio, oracle_lib, numpy_imu, fail_first):
    """INITIAL to the end of a 16-frame stream with the slot fed from the start.  After the hand-over the slot is, bit for bit, the
    restatement of processIMU / processImage / slideWindow over the stream's samples followed by the restatement of init_apply_batch on
    the try's result (with commit_last).  The trajectory is held to the same driver without `state` at tests/test_stream.py's bar
    between two implementations, positions within 1e-3 m and the ATE (ate_rmse) within 1 % (measured 1.23e-4 m, 1.65e-4 m after a
    failed try).  An initialised trajectory lives in the initialisation's frame, so the aligned APE is the sharper figure, and in
    it the two do not fit 1 %: 2.0823e-3 against the slot's 2.0536e-3 m (1.4 %), 2.9228e-3 against 2.8671e-3 m (1.9 %), because the
    driver without `state` linearises its new intervals at zero bias and the slot at their start frame's.  The comparator that shares
    the slot's rule, bias_relinearize= at thresholds that never fire, is held to the bar in both figures: max |dP| 1.95e-7 m and
    9.7e-8 m, APE apart by 2e-9 m and 1.4e-8 m."""
    vs = vio.stream
    plain = vs.StreamDriver(oracle_lib, stream16(vio), seed=2, initialize=dict(scale=3.7, aligner=failing_first(oracle_lib, fail_first)))
    never = vs.StreamDriver(oracle_lib, stream16(vio), seed=2, initialize=dict(scale=3.7, aligner=failing_first(oracle_lib, fail_first)),
                            bias_relinearize=(1e9, 1e9))
    h = fsr.Recording(eir.EstimatorInitReference(vio.synth.preintegrate))
    drv = vs.StreamDriver(oracle_lib, stream16(vio), seed=2, initialize=dict(scale=3.7, aligner=failing_first(oracle_lib, fail_first), state=(h, 0)))
    assert not drv.initialized and h.calls == []            # (the feeding is queued)
    drv.ensure_initialized()
    tries = 2 if fail_first else 1
    assert drv.init_tries == tries and drv.init_frame == 9 + tries
    names = [c[0] for c in h.calls]
    assert names.count("init_apply_batch") == 1 and names.count("slide_batch") == tries - 1
    assert names.count("imu_batch") == names.count("image_batch") == 10 + tries
    res = drv.init_result
    want, status = eir.init_apply(fed_state(vio, drv.s, drv.ext, drv.g_norm, tries - 1), res["poses"], res["speed_bias"], res["g"], res["rot"], commit_last=True)
    assert status == 0
    got = h.state_get(0)
    same_state(want, got)
    assert got["frame_count"] == 10 and np.array_equal(got["lin_bias"][:, 0:3], np.zeros((11, 3))) and np.array_equal(got["lin_bias"][:, 3:6], got["Bgs"])
    assert np.abs(got["Bgs"]).max() > 0 and np.array_equal(got["last_P"], got["Ps"][10])
    tp, tn, td = plain.run(), never.run(), drv.run()
    assert numpy_imu.created == 1 and not hasattr(drv, "imu_h")        # (the comparator's; the slot's side has no IMU-library handle)
    assert len(tp) == len(tn) == len(td) == 16 - drv.init_frame and never.repropagated == [0] * len(tn)
    assert np.array_equal(h.state_get(0)["last_P"], h.state_get(0)["Ps"][10]) and [f["failure"] for f in drv.failures] == [0] * len(td)
    dp, dn = np.abs(td[:, 1:4] - tp[:, 1:4]).max(), np.abs(td[:, 1:4] - tn[:, 1:4]).max()
    ep, en, ed = (vs.ape_stats(t, d.ground_truth())["rmse"] for t, d in ((tp, plain), (tn, never), (td, drv)))
    print("fail_first %s: max |dP| %.3e m (zero-bias intervals) %.3e m (bias_relinearize), aligned APE %.6e %.6e, the slot's %.6e" % (fail_first, dp, dn, ep, en, ed))
    ap, an, ad = (vs.ate_rmse(t, d.ground_truth()) for t, d in ((tp, plain), (tn, never), (td, drv)))
    assert dp < 1e-3 and abs(ad - ap) <= 0.01 * ap          # test_stream.py's bar as it stands there (ate_rmse), against the driver without state
    assert dn < 1e-3 and abs(ad - an) <= 0.01 * an and abs(ed - en) <= 0.01 * en       # ... and with the aligned APE in the ATE's place


def test_a_group_is_fed_and_handed_over_in_one_call_each(vio, oracle_lib):
    """initialize_batched over three drivers on one handle, the second of which fails its first try: the initial feeding is one
    imu_batch and one image_batch per step for the three, the round's two successes are one init_apply_batch, the failure's slide and
    next frame one slide_batch, one imu_batch and one image_batch, and its success the second init_apply_batch.  Each slot equals the
    same driver alone."""
    vs = vio.stream
    base = ir.make_aligner(oracle_lib)
    seen = dict(n=0)

    def aligner(items, intervals, tic, g_norm, noise):
        seen["n"] += 1
        out = base(items, intervals, tic, g_norm, noise)
        if seen["n"] == 1:
            out[1] = dict(status=1)
        return out
    mk = lambda s: vs.SyntheticStream(n_frames=14, seed=s)      # noqa: E731
    h = fsr.Recording(eir.EstimatorInitReference(vio.synth.preintegrate))
    drv = [vs.StreamDriver(oracle_lib, mk(3 + k), seed=2, initialize=dict(scale=2.0, aligner=aligner, state=(h, 7 + k))) for k in range(3)]
    assert vio.batch_stream.initialize_batched(drv) == 2
    assert [d.init_tries for d in drv] == [1, 2, 1]
    assert h.calls == [(n, 3) for _ in range(11) for n in ("imu_batch", "image_batch")] + [("init_apply_batch", 2), ("slide_batch", 1), ("imu_batch", 1),
                                                                                             ("image_batch", 1), ("init_apply_batch", 1)]
    for k, fail in enumerate((False, True, False)):
        one = eir.EstimatorInitReference(vio.synth.preintegrate)
        alone = vs.StreamDriver(oracle_lib, mk(3 + k), seed=2, initialize=dict(scale=2.0, aligner=failing_first(oracle_lib, fail), state=(one, 0)))
        alone.ensure_initialized()
        same_state(one.state_get(0), h.state_get(7 + k))


def biased(vio, n_frames=20):
    """A synthetic stream whose gyroscope and accelerometer carry a constant bias, so that the window's bias estimates move."""
    st = vio.stream.SyntheticStream(n_frames=n_frames, seed=4)
    ba, bg = np.array([0.05, -0.04, 0.03]), np.array([0.004, -0.003, 0.002])
    for k, iv in enumerate(st.imu):
        iv = dict(acc0=iv["acc0"] + ba, gyr0=iv["gyr0"] + bg, dt=list(iv["dt"]), acc=[a + ba for a in iv["acc"]], gyr=[w + bg for w in iv["gyr"]])
        st.imu[k] = iv
        st.preint[k] = vio.synth.preintegrate(iv["acc0"], iv["gyr0"], np.zeros(3), np.zeros(3), iv["dt"], iv["acc"], iv["gyr"])
    return st


RELIN = (0.02, 0.002)


def test_the_slot_relinearises_where_the_driver_would(vio, oracle_lib, numpy_imu):
    """state=dict(relinearize=) against bias_relinearize= without a slot, on a stream with a constant IMU bias: the same number of
    re-propagated intervals at every step, some steps with and some without, and no IMU-library handle on the slot's side.  (Every
    frame is a keyframe: after a non-keyframe slide the two keep different linearisation biases for the merged interval.)"""
    vs = vio.stream
    plain = vs.StreamDriver(oracle_lib, biased(vio), seed=2, bias_relinearize=RELIN)
    assert numpy_imu.created == 1
    tp = plain.run()
    h = fsr.Recording(eir.EstimatorInitReference(vio.synth.preintegrate))
    drv = vs.StreamDriver(oracle_lib, biased(vio), seed=2, state=dict(handle=h, slot=3, relinearize=RELIN))
    td = drv.run()
    assert numpy_imu.created == 1 and not hasattr(drv, "imu_h")
    print("repropagated: driver %s, slot %s" % (plain.repropagated, drv.repropagated))
    assert drv.repropagated == plain.repropagated and len(drv.repropagated) == len(td)
    assert any(n > 0 for n in drv.repropagated) and any(n == 0 for n in drv.repropagated)
    assert [c for c in h.calls if c[0] == "relinearize_batch"] == [("relinearize_batch", 1)] * len(td)
    assert np.abs(td[:, 1:4] - tp[:, 1:4]).max() < 1e-3
    s = h.state_get(3)
    assert np.abs(s["lin_bias"][1:]).max() > 0


def test_the_refusals_stay_and_the_new_forms_are_the_only_way_in(vio, oracle_lib):
    vs = vio.stream
    h = eir.EstimatorInitReference(vio.synth.preintegrate)
    for state in ((h, 0), dict(handle=h, slot=0), dict(handle=h, slot=0, relinearize=RELIN)):
        for kw in (dict(initialize=dict(scale=1.0)), dict(bias_relinearize=(0.1, 0.01)), dict(initialize=dict(scale=1.0, state=(h, 1)))):
            with pytest.raises(ValueError, match="state= cannot be combined"):
                vs.StreamDriver(oracle_lib, stream16(vio), state=state, **kw)
    assert h.state == {}                                    # refused before anything was created
    fm = fsr.NumpyFm(lambda *a: None)
    with pytest.raises(ValueError, match="outlier_px"):
        vs.StreamDriver(oracle_lib, stream16(vio), triangulate=True, outlier_px=3.0, features=(fm, 0), initialize=dict(scale=1.0, state=(h, 0)))
    with pytest.raises(ValueError):
        h.relinearize_batch([(0, -1.0, 0.0)])
    with pytest.raises(ValueError):
        h.init_apply_batch([(0, np.full((11, 7), np.nan), np.zeros((11, 9)), np.zeros(3), np.eye(3))])
    d = vs.StreamDriver(oracle_lib, stream16(vio), seed=2, state=dict(handle=h, slot=2))       # the dict form without relinearize: a state= driver
    assert d.est is h and d.est_slot == 2 and d.est_relin is None and h.state_get(2)["frame_count"] == 10


def test_the_slot_composes_with_features_and_sfm(vio, oracle_lib):
    """Two INITIAL drivers with sfm and their FeatureManagers in slots (the numpy stand-ins), the first failing its first try, through
    initialize_batched with and without estimator-state slots: the same tries, the slots handed over, and the same trajectories to
    tests/test_stream.py's position bar."""
    import sfm_reference as sr
    vs = vio.stream
    sfm = lambda items: [sr.sfm(it) for it in items]       # noqa: E731
    base = ir.make_aligner(oracle_lib)

    def group(est):
        seen = dict(n=0)

        def aligner(items, intervals, tic, g_norm, noise):
            seen["n"] += 1
            out = base(items, intervals, tic, g_norm, noise)
            if seen["n"] == 1:
                out[0] = dict(status=1)
            return out
        ds = []
        for k, seed in enumerate((3, 4)):
            st = vs.SyntheticStream(n_frames=15, landmarks_per_frame=60, track_len=10, seed=seed, pixel_noise=0.1 / 460.0)
            init = dict(sfm=sfm, aligner=aligner)
            if est is not None:
                init["state"] = dict(handle=est, slot=9 + k)
            ds.append(vs.StreamDriver(oracle_lib, st, seed=2, triangulate=True, initialize=init, features=(fm_of[est is not None], 5 + k)))
        assert vio.batch_stream.initialize_batched(ds) == 2
        return ds, [d.run() for d in ds]
    tri = vs.StreamDriver(oracle_lib, stream16(vio), seed=2).ctx.triangulate
    fm_of = {False: fsr.NumpyFm(tri), True: fsr.NumpyFm(tri)}
    h = fsr.Recording(eir.EstimatorInitReference(vio.synth.preintegrate))
    (dp, tp), (dd, td) = group(None), group(h)
    assert [d.init_tries for d in dd] == [d.init_tries for d in dp] == [2, 1]
    assert [c for c in h.calls if c[0] == "init_apply_batch"] == [("init_apply_batch", 1), ("init_apply_batch", 1)]
    for a, b, x, y in zip(dp, dd, tp, td):
        assert a.init_frame == b.init_frame and len(x) == len(y) and not any(f["failure"] for f in b.failures)
        assert np.abs(x[:, 1:4] - y[:, 1:4]).max() < 1e-3
