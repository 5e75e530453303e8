"""readImage for many streams with the forward-backward check on (vio_frame_read_batch behind frame.FrameHandle.set_flow_back; k_front_filter's
three extra ballots) and with rejectWithF off, at full tables: 63 to 1024 rows, the three counts summed over all
sixteen wavefronts, wavefronts and a table in which every row fails the check, k_front_after_reject keeping every one of 900 and more rows.

Two oracles.  The per-stream loop, as in tests/test_gpu_front_back.py: a second handle driven by one FeatureTracker(frames=, rejecter=,
slot=, flow_back=, reject_with_f=) per slot followed by update_ids(), byte for byte on every array and count.  The loop takes its statuses
from the same tracking kernel, so where the rows are tests/flow_back_limits_inputs.full's, n_checked, n_back_lost, n_back_far and
n_after_track are also held to the numpy restatement's own counts: read_batch hands the tracker full's settings (2 levels, the check over
2, half_patch 2, border 1, equalisation off), and the filter's border is the tracker's.  The rig is tests/test_gpu_front_limits.py's
LimitRig with the two settings, its way of seeding a slot's table, and per slot an own camera where one is asked for.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_limits_inputs as bl  # noqa: E402
import flow_back_reference as fb  # noqa: E402
import front_limits_inputs as fl  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402
from test_gpu_front import KEYS, RANSAC  # noqa: E402
from test_gpu_front_cameras import KB, PINHOLE, RecCamera  # noqa: E402
from test_gpu_front_limits import KeepFrames, KeepRejecter, LimitRig  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, WAVE, DT = fl.CAP, fl.WAVE, fl.DT
BACK = dict(levels=2)
NO_BACK = dict(n_checked=0, n_back_lost=0, n_back_far=0)
# tests/test_gpu_front_cameras.py's KANNALA_BRANDT camera at three times the size: the half diagonal, 120 pixels, is 1.48 at mu = 81
KB_BIG = dict(model=KB, width=fl.W, height=fl.H, k2=-0.0125, k3=0.0045, k4=-0.0031, k5=0.00052, mu=81.0, mv=81.6, u0=96.0, v0=72.3, theta_max=1.6)


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_reject(), vio.load_camera()


class BackRig(LimitRig):
    """LimitRig with flow_back and reject_with_f handed to BatchFeatureTracker's handle and to every FeatureTracker of the loop; cams:
    {slot: camera} gives those slots their own camera, and the loop then lifts through a CameraHandle (the other slots through the
    handle's camera as a PINHOLE one).  read() holds the handle to the loop and returns per slot the handle's dict with "back"
    (read_back_info) and "oracle" (n_in, rej, det, the tracker's "status" and the filter's keep mask "filter", None where nothing was
    tracked)."""

    def __init__(self, libs, slots, flow_back=BACK, reject_with_f=True, cams=None, **kw):
        self.flow_back, self.reject_with_f, self.ch = flow_back, bool(reject_with_f), None
        cams = dict(cams or {})
        if cams:
            self.ch = libs[3].create()
            self.ch.set_config(**RANSAC)
            for s in slots:
                self.ch.set_camera(slot=s, **cams.get(s, dict(model=PINHOLE, **fl.CAM)))
        super().__init__(libs[:3], slots, **kw)
        for s, cam in cams.items():
            self.fr.set_slot_camera(s, **cam)
        if flow_back is not None:
            self.fr.set_flow_back(**flow_back)
        if not self.reject_with_f:
            self.fr.set_reject_with_f(False)

    def tracker(self, i):
        rejecter = KeepRejecter(self.rej) if self.ch is None else RecCamera(self.ch, self.slots[i])
        return self.vio.FeatureTracker(None, None, max_cnt=self.max_cnt, min_dist=self.min_dist, border=self.border, mask=self.masks.get(self.slots[i]), rejecter=rejecter,
                                       frames=KeepFrames(self.ofr), slot=self.oslots[i], flow_back=self.flow_back, reject_with_f=self.reject_with_f)

    def close(self):
        super().close()
        if self.ch is not None:
            self.ch.close()

    def set_back(self, **flow_back):
        """Other settings of the check, on the handle and on the loop's."""
        self.flow_back = dict(flow_back)
        self.fr.set_flow_back(**flow_back)
        self.ofr.set_flow_back(**flow_back)
        for ft in self.fts:
            ft.flow_back = self.flow_back

    def read(self, imgs, t, publish=True):
        outs = self.bt.read_images(imgs, t, publish=publish)
        frames = self.bt.feature_frames()
        for i, (ft, o) in enumerate(zip(self.fts, outs)):
            name = ("slot", self.slots[i], "t", t)
            n_in, nr, nd, nt = len(ft.cur_pts), len(ft.rejecter.calls), len(ft.frames.detects), len(ft.frames.tracks)
            ref = ft.read_image(imgs[i], t, publish=publish)
            ref["ids"] = ft.update_ids()
            for key in KEYS:
                same_bytes(o[key], ref[key], name + (key,))
            ids, rows = ft.feature_frame()
            same_bytes(frames[i][0], ids, name + ("feature_frame ids",))
            same_bytes(frames[i][1], rows, name + ("feature_frame rows",))
            assert o["n_new"] == ft.n_new and o["n"] == len(ref["pts"]) and o["n_tracked_in"] == n_in, name
            rej = ft.rejecter.calls[nr] if len(ft.rejecter.calls) > nr else None
            det = ft.frames.detects[nd] if len(ft.frames.detects) > nd else None
            status = keep = None
            if len(ft.frames.tracks) > nt:
                tr = ft.frames.tracks[nt]
                status = tr["status"]
                keep = (status == 0) & ft.in_border(tr["next_pts"], np.asarray(imgs[i]).shape)
            assert o["n_after_track"] == (0 if keep is None else int(keep.sum())), name
            assert (det is not None) == bool(publish) and (self.reject_with_f or rej is None), name
            if publish:
                assert (o["n_after_reject"], o["n_candidates"]) == (det["n_tracked"], det["n_candidates"]), (name, o["n_after_reject"], det)
                active = rej is not None and rej["n"] >= 8
                assert (o["reject_status"], o["reject_hyp"]) == ((rej["status"], rej["hyp"]) if active else (0, -1)), (name, rej)
                if rej is not None:
                    assert rej["n"] == o["n_after_track"], name
            else:
                assert o["n_after_track"] == o["n_after_reject"] == o["n"] and o["n_new"] == 0, name
            o["back"] = self.fr.read_back_info(self.slots[i])
            assert o["back"] == (ft.back_info if self.flow_back is not None else NO_BACK), (name, o["back"], ft.back_info)
            o["oracle"] = dict(n_in=n_in, rej=rej, det=det, status=status, filter=keep)
        return outs

    def seeded_frame(self, rows, publish=True, inverse=0):
        """image(0) unpublished, the slots seeded with the first rows[i] of seeded(1024), then image(1): what full(inverse) restates."""
        self.read([fl.image(0)] * len(self.slots), 0.0, publish=False)
        for i, n in enumerate(rows):
            if n:
                self.seed(i, *fl.seeded(n))
        return self.read([fl.image(1)] * len(self.slots), DT, publish=publish)


def counts(o):
    orc = o["oracle"]
    rej, det = orc["rej"], orc["det"]
    return dict(n_in=orc["n_in"], back=o["back"], after_track=o["n_after_track"], after_reject=o["n_after_reject"],
                reject=None if rej is None else (rej["status"], rej["hyp"]), kept=None if det is None else det["n_kept"], n_new=o["n_new"], n=o["n"])


def restated(inverse, n):
    """(read_back_info's counts, n_after_track, the statuses) of the first n rows of full(inverse)."""
    ref = bl.prefix(bl.full(inverse), n)
    return bl.back_info(ref), fb.counts(ref)["kept"], ref["status"]


# ---- a. a full table against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
def test_full_table_against_the_restatement(libs, inverse):
    """As observed on an MI355X, forward flow (inverse in brackets): frame 1: 1024 rows, 989 (993) checked, 9 (3) lost backwards, 40 (54)
    far, 940 (936) after the filter, which are the restatement's counts; rejectWithF keeps 901 (899), setMask 841 (840) + 183 (184) new.
    Frame 2, not published: 997 (998) checked, 914 (899) kept.  Frame 3: 914 (899) rows in, 859 (838) after the filter."""
    rig = BackRig(libs, [3], equalize=False, inverse=inverse)
    try:
        o = rig.seeded_frame([CAP])[0]
        print("frame 1, inv%d" % inverse, counts(o))
        info, kept, status = restated(inverse, CAP)
        assert min(info["n_back_lost"], info["n_back_far"]) >= 3 and len(bl.failed_groups(bl.full(inverse))) >= 12
        assert o["n_tracked_in"] == CAP and o["back"] == info and o["n_after_track"] == kept, (o["back"], info, o["n_after_track"], kept)
        assert np.array_equal(o["oracle"]["status"], status)
        assert o["oracle"]["rej"]["hyp"] >= 0 and o["n"] == CAP                             # rejectWithF still runs behind the check
        n1 = o["n"]
        o = rig.read([fl.image(2)], 2 * DT, publish=False)[0]
        print("frame 2, not published", counts(o))
        assert o["n_tracked_in"] == n1 and o["back"]["n_checked"] > 512 and o["back"]["n_back_lost"] + o["back"]["n_back_far"] >= 1
        n2 = o["n"]
        o = rig.read([fl.image(3)], 3 * DT)[0]
        print("frame 3", counts(o))
        assert o["n_tracked_in"] == n2 > 512 and o["back"]["n_checked"] > 512 and o["oracle"]["rej"]["hyp"] >= 0 and o["n_new"] > 0
    finally:
        rig.close()


# ---- b. exact row counts in one call -----------------------------------------------------------------------------
SLOTS_B = [0, 7, 31, 100, 200, 255]                     # (31, in the middle, holds no points)


@pytest.mark.parametrize("inverse", [0, 1])
def test_exact_row_counts_in_one_call(libs, inverse):
    """Six streams of one image pair in one read_batch, five of them seeded with prefixes of the same rows: every slot's three counts and
    its n_after_track are those of the restatement's prefix."""
    rows = [63, 64, 0, 65, 1023, 1024]
    rig = BackRig(libs, SLOTS_B, equalize=False, inverse=inverse)
    try:
        outs = rig.seeded_frame(rows)
        for s, n, o in zip(SLOTS_B, rows, outs):
            print("slot %d, inv%d" % (s, inverse), counts(o))
            info, kept, status = restated(inverse, n)
            assert o["n_tracked_in"] == n and o["back"] == info and o["n_after_track"] == kept, (s, o["back"], info, o["n_after_track"], kept)
            if n:
                assert info["n_checked"] > n // 2 and np.array_equal(o["oracle"]["status"], status)
        assert outs[2]["back"] == NO_BACK and outs[2]["n_new"] == outs[2]["n"] > 0
        big = restated(inverse, 1023)[0]
        assert min(big["n_back_lost"], big["n_back_far"]) >= 3
    finally:
        rig.close()


# ---- c. every row fails ------------------------------------------------------------------------------------------
def test_every_row_fails_the_check(libs):
    """max_dist 0: a row is kept only if its backward pass ends on the keypoint's own floats.  Whole wavefronts keep nothing, fewer than 8
    rows reach rejectWithF, so the pair is inactive, and the detection refills the table.  Then the default max_dist on the same handle."""
    rig = BackRig(libs, [6], flow_back=dict(levels=2, max_dist=0.0), equalize=False)
    try:
        o = rig.seeded_frame([CAP])[0]
        print("max_dist 0", counts(o))
        ref = bl.full(0)
        with np.errstate(invalid="ignore"):
            came_back = ref["back_status"] == fb.OK
            exact = came_back & (ref["back_d2"] <= 0.0)
        info = bl.back_info(ref)
        info["n_back_far"] = int(np.sum(came_back & ~exact))                                # the restatement's counts under max_dist 0
        assert o["back"] == info and o["n_after_track"] == int(exact.sum()), (o["back"], info, o["n_after_track"], int(exact.sum()))
        keep = o["oracle"]["filter"]
        empty = [w for w in range(CAP // WAVE) if not keep[w * WAVE:(w + 1) * WAVE].any()]
        print("wavefronts that keep no row: %d" % len(empty))
        assert len(keep) == CAP and len(empty) >= 12
        if o["n_after_track"] < 8:
            assert o["reject_hyp"] == -1 and o["reject_status"] == 0 and o["n_after_reject"] == o["n_after_track"]
        assert o["n"] == CAP and o["n_new"] >= CAP - o["n_after_track"]                     # the detection refills the table
        rig.set_back(levels=2)
        o = rig.read([fl.image(2)], 2 * DT)[0]
        print("the default max_dist again", counts(o))
        assert o["n_tracked_in"] == CAP and o["n_after_track"] > 512 and o["back"]["n_checked"] >= o["n_after_track"]
        assert o["back"]["n_back_lost"] + o["back"]["n_back_far"] >= 1 and o["oracle"]["rej"]["hyp"] >= 0
    finally:
        rig.close()


# ---- d. no rejectWithF at a full table ---------------------------------------------------------------------------
@pytest.mark.parametrize("flow_back", [BACK, None], ids=["check on", "check off"])
def test_without_reject_with_f_at_a_full_table(libs, flow_back):
    """k_front_after_reject keeps every row of more than 900 and hands them to setMask."""
    rig = BackRig(libs, [9], flow_back=flow_back, reject_with_f=False, equalize=False)
    try:
        o = rig.seeded_frame([CAP])[0]
        print(counts(o))
        c = fb.counts(bl.full(0))
        kept = c["kept"] if flow_back is not None else c["forward_ok"]                     # (with the check off: the forward pass's OK rows)
        assert o["n_after_track"] == kept > 900 and o["back"] == (bl.back_info(bl.full(0)) if flow_back is not None else NO_BACK)
        assert o["n_after_reject"] == o["n_after_track"] and o["reject_hyp"] == -1 and o["reject_status"] == 0 and o["oracle"]["rej"] is None
        assert o["oracle"]["det"]["n_tracked"] == kept and 256 < o["oracle"]["det"]["n_kept"] < kept
        assert o["n"] == CAP and o["n_new"] == CAP - o["oracle"]["det"]["n_kept"]           # refilled
        assert len(o["un_pts"]) == CAP and np.all(np.isfinite(o["un_pts"]))                 # every row is published with a lifted point
        o = rig.read([fl.image(2)], 2 * DT)[0]
        print(counts(o))
        assert o["n_after_reject"] == o["n_after_track"] > 512 and o["reject_hyp"] == -1 and np.all(np.isfinite(o["un_pts"]))
    finally:
        rig.close()


# ---- e. a slot with its own camera ---------------------------------------------------------------------------------
def test_full_table_in_a_slot_with_its_own_camera(libs):
    """The second instantiation of csrc/vio_front_body.inc (the slots' own cameras) with the check on, at 1024 rows."""
    slot = 12
    rig = BackRig(libs, [slot], cams={slot: KB_BIG}, equalize=False)
    try:
        o = rig.seeded_frame([CAP])[0]
        print(counts(o))
        info, kept, status = restated(0, CAP)
        assert o["back"] == info and o["n_after_track"] == kept and np.array_equal(o["oracle"]["status"], status)
        assert o["oracle"]["rej"]["n"] == kept and o["oracle"]["rej"]["hyp"] >= 0 and o["reject_hyp"] == o["oracle"]["rej"]["hyp"]
        assert o["n"] == CAP and np.all(np.isfinite(o["un_pts"])) and rig.fr.slot_camera(slot)["model"] == KB
    finally:
        rig.close()
