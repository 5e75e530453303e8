"""readImage for many streams on the device (frame.FrameHandle.read_batch, frontend.BatchFeatureTracker; include/vio_frame_read.h, DESIGN.md
section 24) against the per-step path it replaces: a second handle driven by FeatureTracker(frames=FrameHandle, rejecter=RejectHandle,
slot=s) followed by update_ids(), with the same images, times, camera and settings.  The kernels are the same source and the join is
integer work, so every comparison is byte for byte: pts, ids, track_cnt, un_pts, velocity, n_new and feature_frame().  Every scenario
asserts from the oracle run's own counts that it happened."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as flow_ref  # noqa: E402
import frame_sequences as fs  # noqa: E402
import reject_reference as rr  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

PREV, NEXT = 0, 1
BAD_ARG, FAIL_NO_MODEL = -1, 1
CAM = dict(fx=52.0, fy=51.0, cx=31.5, cy=23.6, k1=-0.12, k2=0.02, p1=3e-4, p2=-2e-4, width=64, height=48)
RANSAC = dict(seed=3, ransac_hypotheses=128, f_threshold=1.0, focal_length=460.0)
MIN_DIST, MAX_CNT, HALF_PATCH, DT = 3, 24, 2, 0.05
KEYS = ("pts", "ids", "track_cnt", "un_pts", "velocity")


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_reject()


class RecRejecter:
    """The RejectHandle behind FeatureTracker's rejecter interface, recording what rejectWithF saw."""

    def __init__(self, rh):
        self.rh, self.calls = rh, []

    def reject(self, cur_pts, forw_pts, pair=0):
        o = self.rh.reject_batch([dict(cur_pts=cur_pts, forw_pts=forw_pts, pair=pair)])[0]
        self.calls.append(dict(n=len(cur_pts), kept=int(o["mask"].sum()), status=o["status"], hyp=o["hyp"], pair=pair))
        return o["mask"]

    def undistort(self, *a, **k):
        return self.rh.undistort(*a, **k)


class RecFrames:
    """The FrameHandle behind FeatureTracker's frames interface, recording what the tracker and the detector saw."""

    def __init__(self, fr):
        self.fr, self.tracks, self.detects = fr, [], []

    def __getattr__(self, k):
        return getattr(self.fr, k)

    def track(self, prev_pts, guess=None, slot=0):
        o = self.fr.track(prev_pts, guess, slot)
        self.tracks.append(dict(n=len(prev_pts), ok=int((o["status"] == 0).sum())))
        return o

    def detect(self, tracked=None, track_cnt=None, max_total=150, slot=0):
        o = self.fr.detect(tracked=tracked, track_cnt=track_cnt, max_total=max_total, slot=slot)
        self.detects.append(dict(n_tracked=len(tracked), n_kept=o["n_kept"], n_new=o["n_new"], n_candidates=o["n_candidates"]))
        return o


class Rig:
    """A handle read through BatchFeatureTracker and an oracle handle read by one FeatureTracker per slot; read() holds the first to the
    second and returns, per slot, the handle's dict with the oracle's counts under "oracle"."""

    def __init__(self, libs, slots, max_cnt=MAX_CNT, border=1, equalize=True, inverse=0, masks=None, oracle_slots=None, cam=None, min_dist=None):
        self.vio, flib, rlib = libs
        self.slots = list(slots)
        self.oslots = list(oracle_slots) if oracle_slots is not None else self.slots
        self.masks = dict(masks or {})
        self.fr, self.ofr, self.rej = flib.create(), flib.create(), rlib.create()
        self.cam, self.min_dist = dict(CAM if cam is None else cam), MIN_DIST if min_dist is None else int(min_dist)
        cfg = dict(equalize=equalize, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow=dict(levels=2, half_patch=HALF_PATCH, inverse=inverse),
                   detect=dict(min_distance=self.min_dist))
        self.fr.set_config(**cfg)
        self.ofr.set_config(**cfg)
        self.fr.set_camera(**self.cam, **RANSAC)
        self.rej.set_camera(**self.cam)
        self.rej.set_config(**RANSAC)
        self.max_cnt, self.border = max_cnt, border
        self.bt = self.vio.BatchFeatureTracker(self.fr, self.slots, max_cnt=max_cnt, min_dist=self.min_dist, border=border, masks=self.masks)
        self.fts = [self.tracker(i) for i in range(len(self.slots))]

    def tracker(self, i):
        return self.vio.FeatureTracker(None, None, max_cnt=self.max_cnt, min_dist=self.min_dist, border=self.border, mask=self.masks.get(self.slots[i]),
                                       rejecter=RecRejecter(self.rej), frames=RecFrames(self.ofr), slot=self.oslots[i])

    def close(self):
        for h in (self.fr, self.ofr, self.rej):
            h.close()

    def set_max_cnt(self, max_cnt):
        self.max_cnt = self.bt.max_cnt = max_cnt
        self.fr.set_tracker(max_cnt=max_cnt, border=self.border)
        for ft in self.fts:
            ft.max_cnt = max_cnt

    def seed(self, i, pts, ids, cnt):
        pts, ids, cnt = np.asarray(pts, np.float32).reshape(-1, 2), np.asarray(ids, np.int64), np.asarray(cnt, np.int32)
        self.fr.points_set(pts, ids, cnt, slot=self.slots[i])
        ft = self.fts[i]
        ft.cur_pts, ft.ids, ft.track_cnt = pts.copy(), ids.copy(), cnt.copy()

    def reset(self, i):
        self.fr.reset(self.slots[i])
        self.ofr.reset(self.oslots[i])
        n_id = self.fts[i].n_id
        self.fts[i] = self.tracker(i)
        self.fts[i].n_id = n_id                                     # (the slot keeps its id counter)

    def direct_push(self, i, img):
        self.fr.push(img, slot=self.slots[i])
        self.ofr.push(img, slot=self.oslots[i])
        ft = self.fts[i]
        ft.cur_pts, ft.ids, ft.track_cnt = np.zeros((0, 2), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int32)

    def read(self, imgs, t, publish=True, which=None):
        which = list(range(len(self.slots))) if which is None else list(which)
        if len(which) == len(self.slots):
            outs = self.bt.read_images(imgs, t, publish=publish)
            frames = self.bt.feature_frames()
        else:
            outs = self.fr.read_batch(imgs, t, slots=[self.slots[i] for i in which], publish=publish)
            frames = [None] * len(which)
        for k, i in enumerate(which):
            ft, o, name = self.fts[i], outs[k], ("slot", self.slots[i], "t", t)
            n_in, nr, nd = len(ft.cur_pts), len(ft.rejecter.calls), len(ft.frames.detects)
            ref = ft.read_image(imgs[k], t, publish=publish)
            ref["ids"] = ft.update_ids()
            for key in KEYS:
                same_bytes(o[key], ref[key], name + (key,))
            assert o["n_new"] == ft.n_new and o["n"] == len(ref["pts"]), name
            if frames[k] is not None:
                ids, rows = ft.feature_frame()
                same_bytes(frames[k][0], ids, name + ("feature_frame ids",))
                same_bytes(frames[k][1], rows, name + ("feature_frame rows",))
            rej = ft.rejecter.calls[nr] if len(ft.rejecter.calls) > nr else None
            det = ft.frames.detects[nd] if len(ft.frames.detects) > nd else None
            assert (det is not None) == bool(publish), name
            orc = dict(n_in=n_in, rej=rej, det=det, n=len(ref["pts"]), n_new=ft.n_new)
            assert o["n_tracked_in"] == n_in, name
            if publish:
                after_track = rej["n"] if rej is not None else 0
                assert (o["n_after_track"], o["n_after_reject"], o["n_candidates"]) == (after_track, det["n_tracked"], det["n_candidates"]), (name, o, orc)
                active = rej is not None and rej["n"] >= 8
                assert (o["reject_status"], o["reject_hyp"]) == ((rej["status"], rej["hyp"]) if active else (0, -1)), (name, o, orc)
            else:
                assert o["n_after_track"] == o["n_after_reject"] == o["n"] and o["n_new"] == 0, name
            o["oracle"] = orc
        return outs


def strong_points(rig, i, img, n, lo, hi):
    """n corners of `img`, the oracle's detector's strongest inside [lo, hi) x [lo, hi): points that track."""
    h = rig.ofr.__class__(rig.ofr.lib)
    try:
        h.set_config(**rig.ofr._cfg)
        h.push(img)
        p = h.detect(max_total=60)["new_pts"]
    finally:
        h.close()
    ok = (p[:, 0] >= lo[0]) & (p[:, 0] < hi[0]) & (p[:, 1] >= lo[1]) & (p[:, 1] < hi[1])
    assert ok.sum() >= n, (ok.sum(), n)
    return p[ok][:n].astype(np.float32)


def out_bytes(outs):
    return [b"".join(o[k].tobytes() for k in KEYS) + repr([o[k] for k in ("n", "n_new", "n_after_track", "n_after_reject", "reject_status",
                                                                         "reject_hyp", "n_candidates")]).encode() for o in outs]


# ---- sequences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alternate", [False, True])
def test_six_frames_on_one_slot(libs, alternate):
    rig = Rig(libs, [5])
    try:
        stats = []
        for t in range(6):
            publish = not alternate or t % 2 == 0
            stats.append(rig.read([fs.image(64, 48, 5, t)], DT * t, publish=publish)[0])
        # the first frame detects, the later ones track; rejectWithF ran its RANSAC; points grew old enough to be published
        assert stats[0]["oracle"]["n_in"] == 0 and stats[0]["n_new"] == stats[0]["n"] > 8
        assert all(s["oracle"]["n_in"] > 0 for s in stats[1:])
        assert any(s["oracle"]["rej"] is not None and s["oracle"]["rej"]["n"] >= 8 for s in stats[1:])
        assert stats[-1]["track_cnt"].max() >= 4
        assert len(rig.bt.feature_frames()[0][0]) > 0
        assert np.any(stats[2]["velocity"] != 0) and np.all(stats[1]["velocity"] == 0)        # the kept quirk: zero in a point's first two frames
        if alternate:
            assert all(s["n_new"] == 0 and s["oracle"]["det"] is None for s in stats[1::2])
    finally:
        rig.close()


def test_five_slots_of_different_geometries(libs):
    shapes, slots = [(64, 48), (61, 45), (129, 17), (33, 9), (17, 13)], [7, 0, 255, 3, 100]
    late, frames = 4, 5
    rig = Rig(libs, slots)
    alone = Rig(libs, slots, oracle_slots=slots)
    moved = Rig(libs, [s ^ 9 for s in slots], oracle_slots=slots)          # every stream in another slot index
    try:
        seen = {i: [] for i in range(5)}
        for t in range(frames):
            which = [i for i in range(5) if i != late or t >= 2]
            imgs = [fs.image(*shapes[i], 20 + i, t - (2 if i == late else 0)) for i in which]
            outs = rig.read(imgs, DT * t, which=which)
            for k, i in enumerate(which):
                seen[i].append(out_bytes([outs[k]])[0])
                if i == late and t in (2, 3):
                    # it joins two frames late: no points to begin with, zero velocities in its first two frames, -1 in prev_un
                    assert (outs[k]["oracle"]["n_in"] == 0) == (t == 2) and outs[k]["n"] > 0
                    assert np.all(outs[k]["velocity"] == 0)
                    if t == 2:
                        assert np.all(rig.fr.points_get(slots[late])["prev_un_ids"] == -1)
        assert any(len(set(s)) > 1 for s in seen.values())
        # each stream alone, in its slot and in another: the same bytes
        for other in (alone, moved):
            for i in range(5):
                got = []
                for t in range(frames):
                    if i == late and t < 2:
                        continue
                    img = fs.image(*shapes[i], 20 + i, t - (2 if i == late else 0))
                    got.append(out_bytes(other.fr.read_batch([img], DT * t, slots=[other.slots[i]]))[0])
                assert got == seen[i], (i, other.slots[i])
    finally:
        for r in (rig, alone, moved):
            r.close()


# ---- the size gate, lost points, a full table -----------------------------------------------------------------
@pytest.mark.parametrize("inside", [7, 8])
def test_size_gate(libs, inside):
    """9 seeded points, 9 - inside of them within the border margin, where they stay whichever way the texture moves: rejectWithF sees 7
    points (the gate: everything is kept) or exactly 8 (its RANSAC runs)."""
    border = 8
    rig = Rig(libs, [2], border=border)
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


def test_every_point_lost(libs):
    """Seeded points, then an unrelated texture.  The tracker has no way to know (Lucas-Kanade converges somewhere: status 0 on the CPU
    restatement too), so the points are seeded where any small step leaves them outside a wide border: none reaches rejectWithF or
    setMask, and the detection fills the table."""
    border = 20
    a, b = fs.image(64, 48, 5, 0), flow_ref.texture(64, 48, seed=99, smooth=1.5)
    pts = np.float32([[12.0 + 5.0 * k, 9.0 if k % 2 else 39.0] for k in range(9)])
    res = flow_ref.multi_level(a, b, pts, None, levels=2, half_patch=HALF_PATCH, inverse=0, order="wave64")
    r = np.rint(res[0].astype(np.float64))
    assert np.all(res[1] == 0) and not np.any((border <= r[:, 0]) & (r[:, 0] < 64 - border) & (border <= r[:, 1]) & (r[:, 1] < 48 - border))
    rig = Rig(libs, [0], border=border, equalize=False)
    try:
        rig.read([a], 0.0, publish=False)
        rig.seed(0, pts, np.arange(9), np.full(9, 3))
        o = rig.read([b], DT)[0]
        assert o["oracle"]["n_in"] == 9 and o["oracle"]["rej"] is None and o["oracle"]["det"]["n_tracked"] == 0
        assert o["n_after_track"] == 0 and o["n_new"] == o["n"] == MAX_CNT and np.all(o["track_cnt"] == 1)
    finally:
        rig.close()


def test_full_table_and_max_cnt_zero(libs):
    probe = Rig(libs, [1])
    rig = Rig(libs, [1])
    try:
        imgs = [fs.image(64, 48, 5, t) for t in range(3)]
        probe.read([imgs[0]], 0.0)
        kept = probe.read([imgs[1]], DT)[0]["oracle"]["det"]["n_kept"]         # what setMask keeps of the tracked points
        assert 0 < kept <= MAX_CNT
        rig.read([imgs[0]], 0.0)
        rig.set_max_cnt(kept)
        o = rig.read([imgs[1]], DT)[0]
        assert o["oracle"]["det"]["n_kept"] == kept and o["oracle"]["det"]["n_new"] == 0 and o["n_new"] == 0 and o["n"] == kept
        rig.set_max_cnt(0)
        o = rig.read([imgs[2]], 2 * DT)[0]
        assert o["oracle"]["n_in"] == kept and o["n_new"] == 0 and o["n"] == o["oracle"]["det"]["n_kept"] > 0
    finally:
        probe.close()
        rig.close()


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("equalize", [False, True])
@pytest.mark.parametrize("kind", [0, 2])
def test_mask(libs, kind, equalize, inverse):
    mask = fs.mask_image(64, 48, kind)
    rig = Rig(libs, [9], equalize=equalize, inverse=inverse, masks={9: mask})
    free = Rig(libs, [9], equalize=equalize, inverse=inverse)
    try:
        for t in range(3):
            o = rig.read([fs.image(64, 48, 5, t)], DT * t)[0]
            p = np.rint(o["pts"][o["n"] - o["n_new"]:]).astype(int)
            assert (o["n_new"] > 0 or t > 0) and np.all(mask[p[:, 1], p[:, 0]] != 0)
        o2 = free.read([fs.image(64, 48, 5, 0)], 0.0)[0]
        p = np.rint(o2["pts"]).astype(int)
        assert np.any(mask[p[:, 1], p[:, 0]] == 0)                            # without the mask, points lie where it is closed
    finally:
        rig.close()
        free.close()


def test_degenerate_pair_keeps_every_point(libs):
    """Nine copies of one point track to nine copies of one point: no scale, no model (VIO_REJECT_FAIL_NO_MODEL on the CPU restatement
    too).  Every point is kept by rejectWithF, and the status is reported; setMask then keeps one."""
    cam = rr.Camera(**CAM)
    assert rr.reject(cam, np.tile(np.float32([[30.2, 20.7]]), (9, 1)), np.tile(np.float32([[31.5, 20.1]]), (9, 1)), 1, RANSAC)["status"] == FAIL_NO_MODEL
    rig = Rig(libs, [0])
    try:
        a, b = fs.image(64, 48, 5, 0), fs.image(64, 48, 5, 1)
        p = strong_points(rig, 0, a, 1, (16, 14), (48, 34))
        rig.read([a], 0.0, publish=False)
        rig.seed(0, np.tile(p, (9, 1)), 50 + np.arange(9), np.full(9, 4))
        o = rig.read([b], DT)[0]
        rej = o["oracle"]["rej"]
        assert rej["n"] == 9 and rej["status"] == FAIL_NO_MODEL and rej["kept"] == 9
        assert o["reject_status"] == FAIL_NO_MODEL and o["n_after_reject"] == 9 and o["oracle"]["det"]["n_kept"] == 1
    finally:
        rig.close()


# ---- slot state -----------------------------------------------------------------------------------------------
def test_reset_then_read_and_a_direct_push(libs):
    rig = Rig(libs, [4])
    try:
        imgs = [fs.image(64, 48, 5, t) for t in range(5)]
        first = rig.read([imgs[0]], 0.0)[0]
        rig.read([imgs[1]], DT)
        top = rig.fr.points_get(4)["next_id"]
        assert top == rig.fts[0].n_id >= first["n"] > 0
        rig.reset(0)
        got = rig.fr.points_get(4)
        assert len(got["pts"]) == 0 and len(got["prev_un_ids"]) == 0 and got["next_id"] == top
        o = rig.read([fs.image(61, 45, 6, 0)], 0.0)[0]                       # another geometry, an earlier time: a new stream
        assert o["oracle"]["n_in"] == 0 and o["n_new"] == o["n"] > 0 and o["ids"].min() == top       # ids go on from the counter
        rig.read([fs.image(61, 45, 6, 1)], DT)
        assert len(rig.fr.points_get(4)["pts"]) > 0
        rig.direct_push(0, fs.image(61, 45, 6, 2))
        assert len(rig.fr.points_get(4)["pts"]) == 0                        # they belonged to the frame that rolled away
        o = rig.read([fs.image(61, 45, 6, 3)], 3 * DT)[0]
        assert o["oracle"]["n_in"] == 0 and o["n_new"] == o["n"] > 0 and np.all(o["velocity"] == 0)
    finally:
        rig.close()


def test_repeated_runs_are_identical(libs):
    runs = []
    for _ in range(2):
        rig = Rig(libs, [0, 8])
        try:
            runs.append([out_bytes(rig.fr.read_batch([fs.image(64, 48, 5, t), fs.image(129, 17, 7, t)], DT * t, slots=[0, 8], publish=t != 2))
                         for t in range(4)])
        finally:
            rig.close()
    assert runs[0] == runs[1] and len({b for r in runs[0] for b in r}) > 4


def snapshot(fr, slot):
    p = fr.points_get(slot)
    return [p[k].tobytes() for k in ("pts", "ids", "track_cnt", "prev_un_ids", "prev_un_pts")] + [p["next_id"], fr.download(slot, PREV).tobytes(),
                                                                                                   fr.download(slot, NEXT).tobytes()]


def test_argument_rules(libs):
    vio, flib, _ = libs
    a, b, c = (fs.image(64, 48, 5, t) for t in range(3))
    fr = flib.create()
    try:
        fr.set_config(equalize=True, flow=dict(levels=2, half_patch=HALF_PATCH), detect=dict(min_distance=MIN_DIST))
        with pytest.raises(vio.VioError) as e:                               # no camera set
            fr.read_batch([a], 0.0, slots=[0])
        assert e.value.status == BAD_ARG and "camera" in str(e.value)
        fr.set_camera(**CAM, **RANSAC)
        fr.set_tracker(max_cnt=MAX_CNT, border=1)
        fr.read_batch([a], 0.0, slots=[0])
        fr.read_batch([b], DT, slots=[0])
        before = snapshot(fr, 0)
        assert len(fr.points_get(0)["pts"]) > 0

        def refused(call, word):
            with pytest.raises(vio.VioError) as e:
                call()
            assert e.value.status == BAD_ARG and word in str(e.value), str(e.value)
            assert snapshot(fr, 0) == before, word

        refused(lambda: fr.read_batch([c, c], 2 * DT, slots=[0, 0]), "twice")
        refused(lambda: fr.read_batch([fs.image(61, 45, 6, 0)], 2 * DT, slots=[0]), "reset")                   # a geometry change
        refused(lambda: fr.read_batch([c], DT, slots=[0]), "time")                                             # a time that does not increase
        refused(lambda: fr.read_batch([c], float("nan"), slots=[0]), "time")
        refused(lambda: fr.read_batch([c, a], [2 * DT, DT], slots=[1, 0]), "time")                                   # ... in a later item: slot 1 stays empty
        refused(lambda: fr.set_tracker(max_cnt=vio.frame.MAX_TRACK_POINTS + 1), "max_cnt")
        pts = fr.points_get(0)
        bad = pts["pts"].copy()
        bad[1, 0] = np.nan
        refused(lambda: fr.points_set(bad, pts["ids"], pts["track_cnt"], slot=0), "finite")
        bad[1, 0] = 64.0                                                                                       # rounds outside the frame
        refused(lambda: fr.points_set(bad, pts["ids"], pts["track_cnt"], slot=0), "outside")
        refused(lambda: fr.points_set(np.zeros((vio.frame.MAX_TRACK_POINTS + 1, 2), np.float32), slot=0), "n must be")
        with pytest.raises(vio.VioError):
            fr.download(1, NEXT)                                                                               # nothing rolled there
        o = fr.read_batch([c], 2 * DT, slots=[0])[0]                                                           # and the stream goes on
        assert o["n_tracked_in"] == len(pts["pts"]) and o["n_after_track"] > 0
    finally:
        fr.close()


def test_counters(libs):
    """Descriptors travel, points do not: the host-to-device bytes of a read besides the image are the same whatever the slot holds."""
    vio, flib, _ = libs
    a, b = fs.image(64, 48, 5, 0), fs.image(64, 48, 5, 1)
    up = {}
    for n in (5, 40):
        fr = flib.create()
        try:
            fr.set_config(equalize=True, flow=dict(levels=2, half_patch=HALF_PATCH), detect=dict(min_distance=MIN_DIST))
            fr.set_camera(**CAM, **RANSAC)
            fr.set_tracker(max_cnt=n, border=1)
            o = fr.read_batch([a], 0.0, slots=[3])[0]
            assert o["n"] == n
            c0 = fr.counters()
            o = fr.read_batch([b], DT, slots=[3])[0]
            c1 = fr.counters()
            assert o["n_tracked_in"] == n
            assert c1["image_up"] - c0["image_up"] == 64 * 48 and c1["image_down"] == c0["image_down"]
            up[n] = c1["other_up"] - c0["other_up"]
            c2 = fr.read_batch([a, b], 2 * DT, slots=[3, 4]) and fr.counters()
            assert c2["image_up"] - c1["image_up"] == 2 * 64 * 48
        finally:
            fr.close()
    assert up[5] == up[40] > 0
