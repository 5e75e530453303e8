"""A camera of its own for every resident slot, of any of the four models (frame.FrameHandle.set_slot_camera, frontend.BatchFeatureTracker's
`cameras`; include/vio_frame_camera.h) against the per-stream path whose results it must equal: a second FrameHandle
driven by one FeatureTracker(frames=, slot=s, rejecter=CameraHandle.bind(s)) per slot followed by update_ids(), with the same images,
times, cameras and RANSAC settings.  The kernels are the same text, so every comparison is byte for byte: pts, ids, track_cnt, un_pts,
velocity, n_new and feature_frame().  Every scenario asserts from the oracle's own counts that what it set out to exercise happened."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_sequences as fs  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402
from test_gpu_front import CAM, DT, HALF_PATCH, KEYS, MAX_CNT, MIN_DIST, RANSAC, RecFrames, snapshot, strong_points  # noqa: E402

pytestmark = pytest.mark.gpu

OK, BAD_ARG, NOT_FINITE = 0, -1, -3
PINHOLE, KB, MEI, SCARAMUZZA = 0, 1, 2, 3
# cameras of tests/test_gpu_camera.py's kind at 64 x 48: the image's half diagonal, 40 pixels, is 1.48 at mu = 27, inside r(1.6) = 1.55
PIN_CAM = dict(model=PINHOLE, **CAM)
KB_CAM = dict(model=KB, width=64, height=48, k2=-0.0125, k3=0.0045, k4=-0.0031, k5=0.00052, mu=27.0, mv=27.2, u0=32.0, v0=24.1, theta_max=1.6)
MEI_CAM = dict(model=MEI, width=64, height=48, xi=0.9, k1=-0.05, k2=0.01, p1=1e-4, p2=-1e-4, gamma1=70.0, gamma2=69.0, u0=31.5, v0=23.6)
SCA_CAM = dict(model=SCARAMUZZA, width=64, height=48, poly0=-22.6, poly1=0.0, poly2=4e-3, ac=0.9995, ad=2.5e-4, ae=-1.5e-4, cx=31.9, cy=24.2)
OTHER_PIN = dict(model=PINHOLE, fx=47.0, fy=48.5, cx=30.2, cy=25.1, k1=0.08, k2=-0.01, p1=-2e-4, p2=1e-4, width=64, height=48)
FOUR = [PIN_CAM, KB_CAM, MEI_CAM, SCA_CAM]
FOUR_SLOTS = [3, 0, 255, 100]
COUNTS = ("status", "n", "n_new", "n_after_track", "n_after_reject", "reject_status", "reject_hyp", "n_candidates", "n_clamped", "n_bad")


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_camera()


class RecCamera:
    """CameraHandle.bind(slot) behind FeatureTracker's rejecter interface, recording what rejectWithF and undistortedPoints gave."""

    def __init__(self, ch, slot):
        self.ch, self.slot, self.calls, self.lifts = ch, slot, [], []

    def reject(self, cur_pts, forw_pts, pair=0):
        o = self.ch.reject_batch([dict(cur_pts=cur_pts, forw_pts=forw_pts, pair=pair, slot=self.slot)])[0]
        self.calls.append(dict(n=len(cur_pts), kept=int(o["mask"].sum()), status=o["status"], hyp=o["hyp"], pair=pair))
        return o["mask"]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        o = self.ch.undistort_batch([dict(pts=pts, ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un_pts, dt=dt, slot=self.slot)])[0]
        self.lifts.append(dict(n=len(pts), status=o["status"], n_clamped=o["n_clamped"]))
        return o["un_pts"], o["velocity"]


def config(fr):
    fr.set_config(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow=dict(levels=2, half_patch=HALF_PATCH), detect=dict(min_distance=MIN_DIST))


class Rig:
    """A handle read through BatchFeatureTracker and an oracle handle read by one FeatureTracker per slot over CameraHandle.bind(slot).
    cams: per slot its own camera, or None for the handle's (handle_cam, include/vio_frame_read.h's keywords), which the oracle takes as a
    PINHOLE camera of the camera library.  read() holds the first to the second."""

    def __init__(self, libs, slots, cams, handle_cam=None, border=1, max_cnt=MAX_CNT):
        self.vio, flib, clib = libs
        self.slots, self.cams = list(slots), list(cams)
        self.fr, self.ofr, self.ch = flib.create(), flib.create(), clib.create()
        config(self.fr)
        config(self.ofr)
        if handle_cam is not None:
            self.fr.set_camera(**handle_cam, **RANSAC)
        else:
            self.fr.set_reject_config(**RANSAC)
        self.ch.set_config(**RANSAC)
        for s, cam in zip(self.slots, self.cams):
            self.ch.set_camera(slot=s, **(cam if cam is not None else dict(model=PINHOLE, **handle_cam)))
        self.max_cnt, self.border = max_cnt, border
        self.bt = self.vio.BatchFeatureTracker(self.fr, self.slots, max_cnt=max_cnt, min_dist=MIN_DIST, border=border,
                                               cameras={s: c for s, c in zip(self.slots, self.cams) if c is not None})
        self.fts = [self.vio.FeatureTracker(None, None, max_cnt=max_cnt, min_dist=MIN_DIST, border=border, rejecter=RecCamera(self.ch, s),
                                            frames=RecFrames(self.ofr), slot=s) for s in self.slots]

    def close(self):
        for h in (self.fr, self.ofr, self.ch):
            h.close()

    def seed(self, i, pts, ids, cnt):
        pts, ids, cnt = np.asarray(pts, np.float32).reshape(-1, 2), np.asarray(ids, np.int64), np.asarray(cnt, np.int32)
        self.fr.points_set(pts, ids, cnt, slot=self.slots[i])
        ft = self.fts[i]
        ft.cur_pts, ft.ids, ft.track_cnt = pts.copy(), ids.copy(), cnt.copy()

    def read(self, imgs, t, publish=True):
        outs = self.bt.read_images(imgs, t, publish=publish)
        frames = self.bt.feature_frames()
        for i, (ft, o) in enumerate(zip(self.fts, outs)):
            name = ("slot", self.slots[i], "t", t)
            n_in, nr, nd, nl = len(ft.cur_pts), len(ft.rejecter.calls), len(ft.frames.detects), len(ft.rejecter.lifts)
            ref = ft.read_image(imgs[i], t, publish=publish)
            ref["ids"] = ft.update_ids()
            for key in KEYS:
                same_bytes(o[key], ref[key], name + (key,))
            assert o["n_new"] == ft.n_new and o["n"] == len(ref["pts"]), name
            ids, rows = ft.feature_frame()
            same_bytes(frames[i][0], ids, name + ("feature_frame ids",))
            same_bytes(frames[i][1], rows, name + ("feature_frame rows",))
            rej = ft.rejecter.calls[nr] if len(ft.rejecter.calls) > nr else None
            det = ft.frames.detects[nd] if len(ft.frames.detects) > nd else None
            und = ft.rejecter.lifts[nl]
            assert o["n_tracked_in"] == n_in and (det is not None) == bool(publish), name
            if publish:
                assert (o["n_after_track"], o["n_after_reject"], o["n_candidates"]) == (rej["n"] if rej else 0, det["n_tracked"], det["n_candidates"]), (name, o)
                active = rej is not None and rej["n"] >= 8
                assert (o["reject_status"], o["reject_hyp"]) == ((rej["status"], rej["hyp"]) if active else (OK, -1)), (name, o, rej)
            # the counts of the undistort stage, as vio_camera_undistort_batch gives them for the same points
            bad = und["status"] == NOT_FINITE
            assert o["n_clamped"] == und["n_clamped"] and (o["n_bad"] > 0) == bad, (name, o["n_clamped"], o["n_bad"], und)
            assert o["status"] == (NOT_FINITE if bad or (rej is not None and rej["status"] == NOT_FINITE) else OK), (name, o["status"], und, rej)
            assert self.fr.read_lift_info(self.slots[i]) == dict(n_clamped=o["n_clamped"], n_bad=o["n_bad"])
            o["oracle"] = dict(n_in=n_in, rej=rej, det=det, und=und)
        return outs


def out_bytes(o):
    return b"".join(o[k].tobytes() for k in KEYS) + repr([o[k] for k in COUNTS]).encode()


def four_images(t):
    return [fs.image(64, 48, 5, t)] * 4                                  # one stream for all four: what differs is the camera


# ---- 1. four slots, four models, one call ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def four_run(libs):
    """Five frames of the four-model call, held to the oracle: per frame the four dicts."""
    rig = Rig(libs, FOUR_SLOTS, FOUR)
    try:
        return [rig.read(four_images(t), DT * t) for t in range(5)]
    finally:
        rig.close()


def test_four_models_in_one_call(four_run):
    for i, cam in enumerate(FOUR):
        stats = [frame[i] for frame in four_run]
        ran = [s["oracle"]["rej"] for s in stats[1:] if s["oracle"]["rej"] is not None and s["oracle"]["rej"]["n"] >= 8]
        assert ran and all(r["hyp"] >= 0 and r["status"] == OK for r in ran), (cam["model"], ran)
        assert any(np.any(s["velocity"] != 0) for s in stats), cam["model"]
        assert all(s["status"] == OK and s["n_bad"] == 0 and s["n_clamped"] == 0 and np.all(np.isfinite(s["un_pts"])) for s in stats)
    for frame in four_run:                                               # the slot reaches the lift: one image, four different un_pts
        assert len({o["un_pts"].tobytes() for o in frame}) == 4
    assert len({o["pts"].tobytes() for o in four_run[0]}) == 1           # (the detection saw one image)


# ---- 2. mixed ownership ---------------------------------------------------------------------------------------
def test_mixed_ownership(libs):
    vio, flib, _ = libs
    rig = Rig(libs, [6, 2], [OTHER_PIN, None], handle_cam=CAM)
    plain = flib.create()                                                # only ever set_camera: the path of include/vio_frame_read.h alone
    try:
        config(plain)
        plain.set_camera(**CAM, **RANSAC)
        plain.set_tracker(max_cnt=MAX_CNT, border=1)
        ran = 0
        for t in range(5):
            imgs = [fs.image(64, 48, 5, t), fs.image(64, 48, 7, t)]
            own, none = rig.read(imgs, DT * t)
            ref = plain.read_batch([imgs[1]], DT * t, slots=[2])[0]
            assert out_bytes(none) == out_bytes(ref), t
            ran += sum(1 for o in (own, none) if o["oracle"]["rej"] is not None and o["oracle"]["rej"]["n"] >= 8 and o["reject_hyp"] >= 0)
        assert ran >= 4 and rig.fr.slot_camera(2) is None and rig.fr.slot_camera(6)["fx"] == 47.0
    finally:
        rig.close()
        plain.close()


# ---- 3. independence --------------------------------------------------------------------------------------------
def test_independence(libs, four_run):
    vio, flib, _ = libs
    seen = [[out_bytes(frame[i]) for frame in four_run] for i in range(4)]

    def run(slots, which):
        fr = flib.create()
        try:
            config(fr)
            fr.set_reject_config(**RANSAC)
            fr.set_tracker(max_cnt=MAX_CNT, border=1)
            for i in which:
                fr.set_slot_camera(slots[i], **FOUR[i])
            return [[out_bytes(o) for o in fr.read_batch([four_images(t)[i] for i in which], DT * t, slots=[slots[i] for i in which])] for t in range(5)]
        finally:
            fr.close()

    again = run(FOUR_SLOTS, range(4))                                    # a second run of the same call
    assert [[f[i] for f in again] for i in range(4)] == seen
    for i in range(4):
        alone = run(FOUR_SLOTS, [i])                                     # the stream alone, in its slot ...
        moved = run([s ^ 9 for s in FOUR_SLOTS], [i])                    # ... and in another slot index
        assert [f[0] for f in alone] == seen[i] and [f[0] for f in moved] == seen[i], i


# ---- 4. the size gate on a fisheye slot -------------------------------------------------------------------------
@pytest.mark.parametrize("inside", [7, 8])
def test_size_gate_on_a_fisheye_slot(libs, inside):
    border = 8
    rig = Rig(libs, [2], [KB_CAM], border=border)
    try:
        a, b = fs.image(64, 48, 5, 0), fs.image(64, 48, 5, 1)
        good = strong_points(rig, 0, a, inside, (16, 14), (48, 34))
        edge = np.float32([[4.0, 14.0 + 9.0 * k] for k in range(9 - inside)])
        rig.read([a], 0.0, publish=False)
        rig.seed(0, np.concatenate([good, edge]), 100 + np.arange(9), 2 + np.arange(9) % 3)
        o = rig.read([b], DT)[0]
        rej = o["oracle"]["rej"]
        assert o["oracle"]["n_in"] == 9 and rej["n"] == inside and o["n_after_track"] == inside
        if inside < 8:
            assert rej["hyp"] == -1 and rej["kept"] == inside and o["n_after_reject"] == inside and o["reject_hyp"] == -1
        else:
            assert rej["hyp"] >= 0 and o["reject_hyp"] == rej["hyp"]
    finally:
        rig.close()


# ---- 5. a lift that fails ---------------------------------------------------------------------------------------
def test_a_lift_that_fails(libs):
    vio, flib, _ = libs
    a, b = fs.image(64, 48, 5, 0), fs.image(64, 48, 5, 1)
    probe = flib.create()                                                # frame 0 as the oracle reads it: the detection does not see a camera
    try:
        config(probe)
        probe.push(a)
        px, py = (float(v) for v in probe.detect(max_total=MAX_CNT)["new_pts"][0])
    finally:
        probe.close()
    assert px == np.floor(px) and py == np.floor(py) and 0 <= px < 64 and 0 <= py < 48       # whole pixels: every product below is exact
    # mx = (px - u0) / 16 = 1, my = 0 and xi = 1: P2 = (1 - mx mx - my my) / 2 == 0
    bad_cam = dict(model=MEI, width=64, height=48, xi=1.0, gamma1=16.0, gamma2=16.0, u0=px - 16.0, v0=py)
    rig = Rig(libs, [4, 9], [bad_cam, KB_CAM])
    try:
        bad, good = rig.read([a, a], 0.0)
        assert tuple(bad["pts"][0]) == (px, py) and bad["oracle"]["und"]["status"] == NOT_FINITE
        assert bad["status"] == NOT_FINITE and bad["n_bad"] >= 1 and bad["n"] > 8
        assert np.all(np.isnan(bad["un_pts"])) and np.all(np.isnan(bad["velocity"]))
        assert np.all(np.isnan(rig.fr.points_get(4)["prev_un_pts"]))
        assert good["status"] == OK and np.all(np.isfinite(good["un_pts"])) and good["n_bad"] == 0
        bad, good = rig.read([b, b], DT)
        rej = bad["oracle"]["rej"]
        assert rej["n"] >= 8 and rej["status"] == NOT_FINITE and rej["kept"] == 0       # the pair's cur lift is bad
        assert (bad["reject_status"], bad["reject_hyp"], bad["n_after_reject"]) == (NOT_FINITE, -1, 0) and bad["status"] == NOT_FINITE
        assert bad["n_new"] == bad["n"] > 0 and np.all(bad["track_cnt"] == 1)           # every tracked point dropped, the detector refills
        assert good["status"] == OK and good["oracle"]["rej"]["hyp"] >= 0 and good["n_after_reject"] > 0
    finally:
        rig.close()


# ---- 6. clamping ------------------------------------------------------------------------------------------------
def test_clamping(libs):
    """theta_max = 0.8: r(0.8) = 0.795 is 21 pixels at mu = 27, and the image's corners lie 40 from the centre."""
    rig = Rig(libs, [1], [dict(KB_CAM, theta_max=0.8)])
    try:
        for t in range(3):
            o = rig.read([fs.image(64, 48, 5, t)], DT * t)[0]
            assert o["n_clamped"] == o["oracle"]["und"]["n_clamped"] > 0 and o["status"] == OK       # (read() compared them too)
            r = np.hypot((o["pts"][:, 0] - 32.0) / 27.0, (o["pts"][:, 1] - 24.1) / 27.2)
            assert o["n_clamped"] >= int(np.sum(r > 0.81)) > 0                  # the points well beyond r(theta_max) are among them
    finally:
        rig.close()


# ---- 7. argument rules ------------------------------------------------------------------------------------------
def test_argument_rules(libs):
    vio, flib, clib = libs
    from vio_amd import camera as cm
    a, b, c = (fs.image(64, 48, 5, t) for t in range(3))
    fr, bare, ch = flib.create(), flib.create(), clib.create()
    try:
        config(fr)
        fr.set_camera(**CAM, **RANSAC)
        fr.set_tracker(max_cnt=MAX_CNT, border=1)
        assert fr.read_lift_info(0) == dict(n_clamped=0, n_bad=0)
        fr.set_slot_camera(0, **KB_CAM)
        fr.read_batch([a, a], 0.0, slots=[0, 1])
        fr.read_batch([b, b], DT, slots=[0, 1])
        before, was = snapshot(fr, 0), fr.slot_camera(0)
        assert was == dict(KB_CAM, k2=KB_CAM["k2"]) and len(fr.points_get(0)["pts"]) > 0

        def refused(call, word):
            with pytest.raises(vio.VioError) as e:
                call()
            assert e.value.status == BAD_ARG and word in str(e.value), str(e.value)
            assert fr.slot_camera(0) == was and snapshot(fr, 0) == before, word

        def unknown_model():                                              # (the binding would refuse it before the library)
            m = cm.VioCameraModel(4, 64, 48, 0, (C.c_double * 16)(*([1.0] * 16)))
            fr._ck(fr.lib.fn["set_slot_camera"](fr.h, C.c_int32(0), C.byref(m)), "set_slot_camera")

        refused(unknown_model, "unknown model")
        refused(lambda: fr.set_slot_camera(0, **dict(KB_CAM, k2=-0.9)), "increase")
        refused(lambda: fr.set_slot_camera(0, **dict(MEI_CAM, gamma1=0.0)), "gamma1")
        refused(lambda: fr.set_slot_camera(256, **KB_CAM), "slot")
        fr.set_slot_camera(0, **MEI_CAM)                                  # a camera that is taken leaves the points alone too
        assert fr.slot_camera(0)["gamma1"] == 70.0 and snapshot(fr, 0) == before
        fr.clear_slot_camera(0)                                           # back to the handle's camera
        assert fr.slot_camera(0) is None and snapshot(fr, 0) == before
        o = fr.read_batch([c], 2 * DT, slots=[0])[0]
        ch.set_camera(slot=0, model=PINHOLE, **CAM)
        same_bytes(o["un_pts"], ch.undistort_batch([dict(pts=o["pts"], ids=o["ids"], slot=0)])[0]["un_pts"], "un_pts after clear")
        fr.reset(0)
        assert fr.read_lift_info(0) == dict(n_clamped=0, n_bad=0)

        # a listed slot without any camera: the whole call is refused, and nothing is written, launched or rolled
        config(bare)
        bare.set_tracker(max_cnt=MAX_CNT, border=1)
        with pytest.raises(vio.VioError) as e:
            bare.read_batch([a], 0.0, slots=[0])
        assert e.value.status == BAD_ARG and "camera" in str(e.value)
        bare.set_reject_config(**RANSAC)
        bare.set_slot_camera(0, **KB_CAM)
        for t, img in enumerate((a, b)):
            bare.read_batch([img], DT * t, slots=[0])
            bare.push(img, slot=2)                                       # frames, but no camera
        assert len(bare.points_get(0)["pts"]) > 0
        snaps, counters = [snapshot(bare, s) for s in (0, 2)], bare.counters()
        for slots in ([0, 2], [2, 0], [2]):
            with pytest.raises(vio.VioError) as e:
                bare.read_batch([c] * len(slots), 2 * DT, slots=slots)
            assert e.value.status == BAD_ARG and "slot 2 has no camera" in str(e.value), str(e.value)
            assert bare.counters() == counters
        assert [snapshot(bare, s) for s in (0, 2)] == snaps
        with pytest.raises(vio.VioError):
            bare.set_reject_config(ransac_hypotheses=0)
        o = bare.read_batch([c], 2 * DT, slots=[0])[0]                    # and the stream goes on
        assert o["n_tracked_in"] > 0 and o["status"] == OK
    finally:
        for h in (fr, bare, ch):
            h.close()
