"""The forward-backward check and the rejectWithF switch in readImage for many streams (include/vio_frame_back.h; frame.FrameHandle
.set_flow_back, .set_reject_with_f, .read_back_info; frontend.BatchFeatureTracker(flow_back=, reject_with_f=)) against the per-step path: a
second handle driven by one FeatureTracker(frames=, rejecter=CameraHandle.bind(slot), slot=, flow_back=, reject_with_f=) per slot
followed by update_ids(), with the same images, times, cameras and settings.  Every array agrees byte for byte, and the check's counts
are the loop's own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_sequences as fs  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402
from test_gpu_front import CAM, DT, KEYS, MAX_CNT, MIN_DIST, RANSAC, RecFrames, snapshot  # noqa: E402
from test_gpu_front_cameras import KB_CAM, PINHOLE, RecCamera, config  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG = -1
SLOTS, SEEDS = [4, 0, 200], [31, 32, 33]
BACK = dict(levels=2)


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_camera()


class Rig:
    """A handle read through BatchFeatureTracker(flow_back=, reject_with_f=) and an oracle handle read by one FeatureTracker per slot
    with the same two arguments; cams: per slot its own camera, or None for the handle's."""

    def __init__(self, libs, cams, flow_back=BACK, reject_with_f=True):
        self.vio, flib, clib = libs
        self.fr, self.ofr, self.ch = flib.create(), flib.create(), clib.create()
        config(self.fr)
        config(self.ofr)
        self.fr.set_camera(**CAM, **RANSAC)
        self.ch.set_config(**RANSAC)
        for s, cam in zip(SLOTS, cams):
            self.ch.set_camera(slot=s, **(cam if cam is not None else dict(model=PINHOLE, **CAM)))
        self.bt = self.vio.BatchFeatureTracker(self.fr, SLOTS, max_cnt=MAX_CNT, min_dist=MIN_DIST, cameras={s: c for s, c in zip(SLOTS, cams) if c is not None},
                                               flow_back=flow_back, reject_with_f=reject_with_f)
        self.fts = [self.vio.FeatureTracker(None, None, max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=RecCamera(self.ch, s), frames=RecFrames(self.ofr),
                                            slot=s, flow_back=flow_back, reject_with_f=reject_with_f) for s in SLOTS]

    def close(self):
        for h in (self.fr, self.ofr, self.ch):
            h.close()

    def read(self, t, publish=True):
        imgs = [fs.image(64, 48, seed, t) for seed in SEEDS]
        outs = self.bt.read_images(imgs, DT * t, publish=publish)
        frames = self.bt.feature_frames()
        for i, (ft, o) in enumerate(zip(self.fts, outs)):
            name = ("slot", SLOTS[i], "t", t)
            n_in, nr = len(ft.cur_pts), len(ft.rejecter.calls)
            ref = ft.read_image(imgs[i], DT * t, publish=publish)
            ref["ids"] = ft.update_ids()
            for key in KEYS:
                same_bytes(o[key], ref[key], name + (key,))
            ids, rows = ft.feature_frame()
            same_bytes(frames[i][0], ids, name + ("feature_frame ids",))
            same_bytes(frames[i][1], rows, name + ("feature_frame rows",))
            assert o["n_new"] == ft.n_new and o["n"] == len(ref["pts"]) and o["n_tracked_in"] == n_in, name
            o["back"] = self.fr.read_back_info(SLOTS[i])
            o["rejected"] = len(ft.rejecter.calls) > nr
            if ft.flow_back is not None:
                assert o["back"] == ft.back_info, (name, o["back"], ft.back_info)
            else:
                assert o["back"] == dict(n_checked=0, n_back_lost=0, n_back_far=0), name
        return outs


@pytest.mark.parametrize("cams", [[None, None, None], [None, KB_CAM, None]], ids=["handle camera", "one KANNALA_BRANDT slot"])
def test_batched_against_the_loop(libs, cams):
    rig = Rig(libs, cams)
    try:
        failed = checked = 0
        for t in range(4):
            outs = rig.read(t, publish=t != 2)
            for ft, o in zip(rig.fts, outs):
                b = ft.back_info                                    # the loop's own counts
                failed += b["n_back_lost"] + b["n_back_far"]
                checked += b["n_checked"]
                assert b["n_checked"] - b["n_back_lost"] - b["n_back_far"] >= o["n_after_track"]
                if t != 2 and o["n_after_track"] >= 8:
                    assert o["rejected"] and o["reject_hyp"] >= 0   # rejectWithF still runs behind the check
            print("t %d: %s" % (t, [o["back"] for o in outs]))
        assert checked > 0 and failed >= 1, (checked, failed)
    finally:
        rig.close()


@pytest.mark.parametrize("flow_back", [BACK, None], ids=["check on", "check off"])
def test_without_reject_with_f(libs, flow_back):
    rig = Rig(libs, [None, KB_CAM, None], flow_back=flow_back, reject_with_f=False)
    on = Rig(libs, [None, KB_CAM, None], flow_back=flow_back)
    try:
        for t in range(4):
            publish = t != 2
            outs = rig.read(t, publish=publish)
            stage = rig.fr.read_timing()["reject_ms"]
            on.read(t, publish=publish)
            stage_on = on.fr.read_timing()["reject_ms"]
            for o in outs:
                assert o["n_after_reject"] == o["n_after_track"] and o["reject_hyp"] == -1 and o["reject_status"] == 0 and not o["rejected"], o
                assert len(o["un_pts"]) == o["n"] and np.all(np.isfinite(o["un_pts"]))         # undistortedPoints runs as always
            if t >= 1:
                assert any(o["n_after_track"] >= 8 for o in outs)                           # pairs rejectWithF would have taken
            # the reject stage of vio_frame_read_timing is two event records with no launch between them, as in an unpublished read;
            # behind a RANSAC launch it is 1.6 ms or more
            print("t %d: reject stage %.4f ms without rejectWithF, %.4f ms with it" % (t, stage, stage_on))
            assert stage < 0.1, stage
            if publish and t >= 1:
                assert stage_on > 4 * stage, (stage_on, stage)
    finally:
        rig.close()
        on.close()


def test_argument_rules(libs):
    vio, flib, _ = libs
    fr = flib.create()
    try:
        config(fr)                                                  # 2 flow levels
        fr.set_camera(**CAM, **RANSAC)
        img0, img1 = fs.image(64, 48, 31, 0), fs.image(64, 48, 31, 1)
        fr.read_batch([img0], 0.0, slots=[6])
        fr.set_flow_back(levels=2, max_dist=0.25)
        fr.read_batch([img1], DT, slots=[6])
        pts = fr.points_get(6)["pts"]
        assert len(pts) > 0
        want = fr.track(pts[:5], slot=6, back=True)
        was, info = snapshot(fr, 6), fr.read_back_info(6)

        def refused(call):
            with pytest.raises(vio.VioError) as e:
                call()
            assert e.value.status == BAD_ARG, e.value
            assert snapshot(fr, 6) == was and fr.read_back_info(6) == info
            got = fr.track(pts[:5], slot=6, back=True)              # the settings are what they were: 2 levels, 0.25
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), k

        refused(lambda: fr.set_flow_back(levels=3))
        refused(lambda: fr.set_flow_back(max_dist=-0.5))
        refused(lambda: fr.set_config(flow=dict(levels=1, half_patch=2)))      # below the check's levels
        fr.set_flow_back(enabled=False)
        with pytest.raises(vio.VioError) as e:
            fr.track(pts[:5], slot=6, back=True)
        assert e.value.status == BAD_ARG
        assert snapshot(fr, 6) == was
        with pytest.raises(vio.VioError) as e:
            fr._ck(fr.lib.fn["set_reject_with_f"](fr.h, 2), "set_reject_with_f")
        assert e.value.status == BAD_ARG
        fr.reset(6)
        assert fr.read_back_info(6) == dict(n_checked=0, n_back_lost=0, n_back_far=0)
    finally:
        fr.close()
