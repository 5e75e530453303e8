"""The prediction in the front end on the GPU: FeatureTracker.read_image after set_prediction equals
FlowHandle.track(guess=composed) byte for byte, the same through frames= with FrameHandle.track, the frame after equals an unpredicted
one, and frontend.predict_pixels over a seeded FmHandle slot and a CameraHandle equals the two restatements chained.  The images are
the 96 x 72 fixture of the forward-backward tests (tests/flow_back_reference.py's fixture(), generated here anew): the second image is the
first shifted by (3, 2), so a guess near the shift is a better start than the old pixel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_project_reference as cp  # noqa: E402
import camera_reference as cr  # noqa: E402
import flow_back_reference as fb  # noqa: E402
import fm_predict_reference as fp  # noqa: E402
import predict_inputs as pi  # noqa: E402

pytestmark = pytest.mark.gpu
L = fb.FIXTURE_LEVELS
MAX_CNT, MIN_DIST = 60, 7
KEYS = ("next_pts", "status", "iterations", "cost")


class Rec:
    """A handle behind FeatureTracker's tracker or frames interface that records every track call: its arguments and what it returned."""

    def __init__(self, h):
        self.h, self.calls = h, []

    def __getattr__(self, k):
        return getattr(self.h, k)

    def track(self, *a, **kw):
        o = self.h.track(*a, **kw)
        self.calls.append(dict(args=[np.array(x) if isinstance(x, np.ndarray) else x for x in a], kw=dict(kw), out=o))
        return o


def same(got, ref, name):
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), (name, k)


def compose(cur, ids, pred_ids, pred_px):
    """The rule, written out apart from the front end: the predicted pixel where the point's id is listed, its own pixel otherwise."""
    g = np.array(cur, dtype=np.float32)
    table = {int(i): p for i, p in zip(pred_ids[::-1], np.asarray(pred_px, dtype=np.float32)[::-1])}
    for k, i in enumerate(ids):
        if int(i) >= 0 and int(i) in table:
            g[k] = table[int(i)]
    return g


def prediction_for(ft):
    """Predicted pixels for two thirds of the current points: the true shift (3, 2) plus a fraction of a pixel; and two ids no point
    has."""
    ids, cur = ft.ids.copy(), ft.cur_pts.copy()
    rng = np.random.RandomState(5)
    pick = np.nonzero(rng.uniform(size=len(ids)) < 0.67)[0]
    px = cur[pick].astype(np.float64) + [3.0, 2.0] + rng.uniform(-0.4, 0.4, (len(pick), 2))
    return np.concatenate([ids[pick][::-1], [10 ** 6, -7]]), np.concatenate([px[::-1], [[5.0, 5.0], [6.0, 6.0]]])


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_flow(), vio.load_detect(), vio.load_frame()


@pytest.mark.parametrize("inverse", [0, 1])
def test_read_image_after_set_prediction_is_track_with_the_composed_guess(libs, inverse):
    vio, flow, detect, _ = libs
    a, b, _ = fb.fixture()
    fh, dh = flow.create(), detect.create()
    try:
        fh.set_config(levels=L, inverse=inverse)
        rec = Rec(fh)
        ft = vio.FeatureTracker(rec, dh, max_cnt=MAX_CNT, min_dist=MIN_DIST)
        ft.read_image(a, 0.0)
        ft.update_ids()
        assert len(ft.ids) >= 30 and not rec.calls
        cur, ids = ft.cur_pts.copy(), ft.ids.copy()
        pred_ids, pred_px = prediction_for(ft)
        ft.set_prediction(pred_ids, pred_px)
        out = ft.read_image(b, 1.0)
        assert len(rec.calls) == 1 and list(rec.calls[0]["kw"]) == ["guess"]
        guess = compose(cur, ids, pred_ids, pred_px)
        assert rec.calls[0]["kw"]["guess"].tobytes() == guess.tobytes() and ft.pred_info["n_guessed"] == len(pred_ids) - 2
        assert np.any(guess != cur) and np.any(np.all(guess == cur, axis=1))
        direct = fh.track(a, b, cur, guess=guess)
        same(rec.calls[0]["out"], direct, "guessed frame")
        plain = fh.track(a, b, cur)
        assert direct["next_pts"].tobytes() != plain["next_pts"].tobytes()        # the guess was used
        # what read_image kept are points that call tracked, where it put them (setMask thins them by min_dist afterwards)
        ok = (direct["status"] == 0) & ft.in_border(direct["next_pts"], b.shape)
        kept = np.nonzero(out["ids"] >= 0)[0]
        assert len(kept) >= 20 and np.all(np.isin(out["ids"][kept], ids[ok]))
        where = {int(i): k for k, i in enumerate(ids)}
        assert all(out["pts"][k].tobytes() == direct["next_pts"][where[int(out["ids"][k])]].tobytes() for k in kept)
        ft.update_ids()
        # the frame after: no guess, and the bytes of an unpredicted call
        cur2 = ft.cur_pts.copy()
        ft.read_image(a, 2.0)
        assert len(rec.calls) == 2 and rec.calls[1]["kw"] == {} and len(rec.calls[1]["args"]) == 3
        same(rec.calls[1]["out"], fh.track(b, a, cur2), "the frame after")
    finally:
        fh.close()
        dh.close()


def test_the_same_through_frames(libs):
    vio, _, _, frame = libs
    a, b, _ = fb.fixture()
    fr = frame.create()
    try:
        fr.set_config(equalize=False, flow=dict(levels=L))
        rec = Rec(fr)
        ft = vio.FeatureTracker(None, None, max_cnt=MAX_CNT, min_dist=MIN_DIST, frames=rec, slot=2)
        ft.read_image(a, 0.0)
        ft.update_ids()
        assert len(ft.ids) >= 30 and not rec.calls
        cur, ids = ft.cur_pts.copy(), ft.ids.copy()
        pred_ids, pred_px = prediction_for(ft)
        ft.set_prediction(pred_ids, pred_px)
        ft.read_image(b, 1.0)
        assert len(rec.calls) == 1 and sorted(rec.calls[0]["kw"]) == ["guess", "slot"] and rec.calls[0]["kw"]["slot"] == 2
        guess = compose(cur, ids, pred_ids, pred_px)
        assert rec.calls[0]["kw"]["guess"].tobytes() == guess.tobytes()
        direct = fr.track(cur, guess=guess, slot=2)          # (the slot still holds a and b)
        same(rec.calls[0]["out"], direct, "guessed frame through frames=")
        assert direct["next_pts"].tobytes() != fr.track(cur, slot=2)["next_pts"].tobytes()
        ft.update_ids()
        cur2 = ft.cur_pts.copy()
        ft.read_image(a, 2.0)
        assert len(rec.calls) == 2 and sorted(rec.calls[1]["kw"]) == ["slot"]
        same(rec.calls[1]["out"], fr.track(cur2, slot=2), "the frame after through frames=")
    finally:
        fr.close()


def test_fallback_on_the_device(libs):
    """A prediction that sends every point far off: fewer than min_tracked come back, and the frame is tracked again from the old
    pixels, with the bytes of an unpredicted frame."""
    vio, flow, detect, _ = libs
    a, b, _ = fb.fixture()
    fh, dh = flow.create(), detect.create()
    try:
        fh.set_config(levels=L)
        rec = Rec(fh)
        ft = vio.FeatureTracker(rec, dh, max_cnt=MAX_CNT, min_dist=MIN_DIST, prediction=dict(min_tracked=10 ** 6))
        ft.read_image(a, 0.0)
        ft.update_ids()
        cur, ids0 = ft.cur_pts.copy(), ft.ids.copy()
        ft.set_prediction(ft.ids, cur + 1.0)
        out = ft.read_image(b, 1.0)
        assert len(rec.calls) == 2 and list(rec.calls[0]["kw"]) == ["guess"] and rec.calls[1]["kw"] == {} and ft.pred_info["fell_back"]
        plain = fh.track(a, b, cur)
        same(rec.calls[1]["out"], plain, "fallback")
        ok = (plain["status"] == 0) & ft.in_border(plain["next_pts"], b.shape)
        kept = out["ids"][out["ids"] >= 0]
        assert len(kept) >= 20 and np.all(np.isin(kept, ids0[ok]))
    finally:
        fh.close()
        dh.close()


@pytest.mark.parametrize("name,params", [("pinhole", cr.EUROC), ("kb", cr.KB_FOUR), ("scaramuzza", cr.SCARAMUZZA)])
def test_predict_pixels_is_the_two_restatements_chained(libs, name, params):
    vio = libs[0]
    fmh, ch = vio.load_fm().create(), vio.load_camera().create()
    try:
        cam = cr.Camera(**params)
        inv = cp.fit_inv_poly(cam) if cam.model == cr.MODEL_SCARAMUZZA else None
        ch.set_camera(slot=4, **params)
        if inv is not None:
            ch.set_inv_poly(4, inv)
        poses, ext, nxt = pi.poses(8)
        t, _ = pi.table(257, 10)
        fmh.tracks_set(6, *[t[k] for k in ("ids", "start", "depth", "flag", "off", "pts")])
        for nx in (None, nxt):
            ids, pix = vio.frontend.predict_pixels(fmh, ch, 10, poses, ext, next_pose=nx, fm_slot=6, camera_slot=4, width=cam.width, height=cam.height)
            w_ids, w_pts, _, _ = fp.predict(t, 10, poses, ext, nx)
            w_pix, w_flags = cp.project(cam, w_pts, inv)
            with np.errstate(invalid="ignore"):
                ok = (w_flags == 0) & (w_pix[:, 0] >= 0) & (w_pix[:, 0] <= cam.width - 1) & (w_pix[:, 1] >= 0) & (w_pix[:, 1] <= cam.height - 1)
            assert np.array_equal(ids, w_ids[ok]) and pix.tobytes() == w_pix[ok].tobytes()
            assert len(ids) > 0 and (name == "kb" or len(ids) < len(w_ids)), (len(ids), len(w_ids))      # some predictions leave the image
            all_ids, all_pix = vio.frontend.predict_pixels(fmh, ch, 10, poses, ext, next_pose=nx, fm_slot=6, camera_slot=4)
            assert np.array_equal(all_ids, w_ids[w_flags == 0]) and all_pix.tobytes() == w_pix[w_flags == 0].tobytes()
    finally:
        fmh.close()
        ch.close()
