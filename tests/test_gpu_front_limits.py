"""readImage for many streams on the device (frame.FrameHandle.read_batch; include/vio_frame_read.h) where a
slot's points outnumber a wavefront and fill the workgroup: tables of 63 to 1024 rows, compactions that drop rows in many of the
sixteen wavefronts or whole wavefronts, flow offsets that are no multiple of 4 or 64, rejectWithF striding over its input, setMask over
more tracked points than it has threads, the id lookup over one full chunk, more rows than max_cnt.

The oracle is tests/test_gpu_front.py's: a second handle driven per stream by FeatureTracker(frames=FrameHandle, rejecter=RejectHandle,
slot=s) followed by update_ids(), the per-stage kernels that the other suites hold to the numpy restatements.  Rig.read compares pts,
ids, track_cnt, un_pts, velocity, the counts and feature_frame() byte for byte; there is no tolerance.  Every scenario asserts from the
oracle's recorded arrays that what it names happened.  The inputs are tests/front_limits_inputs.py's, which
tests/test_front_limits_inputs_cpu.py holds to the numpy restatements without a GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_sequences as fs  # noqa: E402
import front_limits_inputs as fl  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402
from test_gpu_front import RecFrames, RecRejecter, Rig, out_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, WAVE, DT = fl.CAP, fl.WAVE, fl.DT


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_reject()


class KeepRejecter(RecRejecter):
    """RecRejecter that keeps rejectWithF's mask."""

    def reject(self, cur_pts, forw_pts, pair=0):
        mask = super().reject(cur_pts, forw_pts, pair)
        self.calls[-1]["mask"] = np.asarray(mask).astype(bool)
        return mask


class KeepFrames(RecFrames):
    """RecFrames that keeps the tracker's status array and positions and setMask's keep_order."""

    def track(self, prev_pts, guess=None, slot=0):
        o = super().track(prev_pts, guess, slot)
        self.tracks[-1].update(status=o["status"].copy(), next_pts=o["next_pts"].copy())
        return o

    def detect(self, tracked=None, track_cnt=None, max_total=150, slot=0):
        o = super().detect(tracked=tracked, track_cnt=track_cnt, max_total=max_total, slot=slot)
        self.detects[-1]["keep_order"] = o["keep_order"].copy()
        return o


class LimitRig(Rig):
    """Rig with the camera and min_distance of the 192 x 144 streams and the recorders above; read() adds under "oracle" the filter's
    keep mask ("filter": the tracker's status 0 and inside the border, None where nothing was tracked)."""

    def __init__(self, libs, slots, max_cnt=CAP, border=fl.BORDER, min_dist=fl.MIN_DIST, **kw):
        super().__init__(libs, slots, max_cnt=max_cnt, border=border, cam=fl.CAM, min_dist=min_dist, **kw)

    def tracker(self, i):
        return self.vio.FeatureTracker(None, None, max_cnt=self.max_cnt, min_dist=self.min_dist, border=self.border, mask=self.masks.get(self.slots[i]),
                                       rejecter=KeepRejecter(self.rej), frames=KeepFrames(self.ofr), slot=self.oslots[i])

    def read(self, imgs, t, publish=True, which=None):
        idx = list(range(len(self.slots))) if which is None else list(which)
        before = [len(self.fts[i].frames.tracks) for i in idx]
        outs = super().read(imgs, t, publish=publish, which=which)
        for k, i in enumerate(idx):
            ft, keep = self.fts[i], None
            if len(ft.frames.tracks) > before[k]:
                tr = ft.frames.tracks[before[k]]
                keep = (tr["status"] == 0) & ft.in_border(tr["next_pts"], np.asarray(imgs[k]).shape)
                assert int(keep.sum()) == outs[k]["n_after_track"], (self.slots[i], t)
            outs[k]["oracle"]["filter"] = keep
        return outs


def counts(o):
    orc = o["oracle"]
    rej, det = orc["rej"], orc["det"]
    return dict(n_in=orc["n_in"], after_track=o["n_after_track"], after_reject=o["n_after_reject"],
                reject=None if rej is None else (rej["status"], rej["hyp"]), kept=None if det is None else det["n_kept"],
                n_new=o["n_new"], n=o["n"])


# ---- a. a full table through five frames -------------------------------------------------------------------------
@pytest.mark.parametrize("equalize,inverse", [(False, 0), (False, 1), (True, 0)])
def test_full_table_through_five_frames(libs, equalize, inverse):
    """As observed on an MI355X, equalize off and the forward flow (rows in -> after the filter -> after rejectWithF -> after setMask +
    new = rows): frame 0: 0 -> 1024 new; 1: 1024 -> 989 -> 917 -> 853 + 171 = 1024; 2: 1024 -> 998 -> 899 -> 850 + 174 = 1024; 3, not
    published: 1024 -> 997; 4: 997 -> 988 -> 880 -> 836 + 188 = 1024.  Every frame's counts are printed."""
    slot = 3
    rig = LimitRig(libs, [slot], equalize=equalize, inverse=inverse)
    try:
        o = rig.read([fl.image(0)], 0.0)[0]
        print("frame 0", counts(o))
        assert o["n_new"] == o["n"] == CAP and np.array_equal(o["ids"], np.arange(CAP))

        o = rig.read([fl.image(1)], DT)[0]
        print("frame 1", counts(o))
        orc = o["oracle"]
        keep, rej, det = orc["filter"], orc["rej"], orc["det"]
        assert o["n_tracked_in"] == CAP and len(keep) == CAP
        assert keep.sum() > 512 and len(fl.waves_with_drops(keep)) >= 4
        assert rej["n"] == keep.sum() and rej["status"] == 0 and rej["hyp"] >= 0 and o["reject_hyp"] == rej["hyp"]      # active and OK
        assert rej["kept"] > 512 and len(fl.waves_with_drops(rej["mask"])) >= 4
        assert det["n_tracked"] == rej["kept"] > 256                                # setMask: a thread owns several entries
        assert det["n_kept"] < det["n_tracked"] and not np.array_equal(det["keep_order"], np.arange(det["n_kept"]))
        assert o["n_new"] > 0 and o["n"] == CAP

        before = rig.fr.points_get(slot)
        assert len(before["prev_un_ids"]) == CAP and before["next_id"] == rig.fts[0].n_id     # m == 1024: the id lookup's one full chunk
        o = rig.read([fl.image(2)], 2 * DT)[0]
        print("frame 2", counts(o))
        assert o["n_tracked_in"] == CAP and np.count_nonzero(np.any(o["velocity"] != 0, axis=1)) > 512
        assert o["n_new"] > 0 and np.array_equal(o["ids"][o["n"] - o["n_new"]:], before["next_id"] + np.arange(o["n_new"]))
        assert rig.fr.points_get(slot)["next_id"] == before["next_id"] + o["n_new"]

        n2 = o["n"]
        o = rig.read([fl.image(3)], 3 * DT, publish=False)[0]                       # the merge reads the unfiltered arrays
        print("frame 3", counts(o))
        assert o["n_tracked_in"] == n2 > 512 and o["n"] == o["oracle"]["filter"].sum() > 512 and o["oracle"]["det"] is None
        assert len(fl.waves_with_drops(o["oracle"]["filter"])) >= 4

        n3 = o["n"]
        o = rig.read([fl.image(4)], 4 * DT)[0]                                      # published again
        print("frame 4", counts(o))
        assert o["n_tracked_in"] == n3 and o["oracle"]["rej"]["hyp"] >= 0 and o["oracle"]["det"]["n_kept"] > 256 and o["n_new"] > 0
        assert o["track_cnt"].max() == 5
    finally:
        rig.close()


# ---- b. exact row counts in one call -----------------------------------------------------------------------------
SLOTS_B = [0, 7, 100, 31, 200, 9, 255]                  # (31, in the middle, holds no points)


@pytest.mark.parametrize("first", [63, CAP])
def test_exact_row_counts_in_one_call(libs, first):
    """Seven streams in one read_batch, six of them seeded: the items' offsets into the call's flat keypoint list are 63, 127, 192, 192,
    447, 704 (or 1024, 1088, ...), and every table ends inside a wavefront, at its edge or one past it."""
    rows = [first, 64, 65, 0, 255, 257, 1023]
    offs = np.cumsum(rows)[:-1].tolist()
    assert offs == ([63, 127, 192, 192, 447, 704] if first == 63 else [1024, 1088, 1153, 1153, 1408, 1665])
    assert sum(o % 4 != 0 for o in offs) >= 3 and sum(o % WAVE != 0 for o in offs) >= 3
    seeds = [fl.SEED + i for i in range(len(rows))]
    a = [fl.image(0, s) for s in seeds]
    b = [fl.image(1, s) for s in seeds]
    rig = LimitRig(libs, SLOTS_B)
    alone = LimitRig(libs, SLOTS_B)
    moved = LimitRig(libs, [s ^ 9 for s in SLOTS_B])
    try:
        rig.read(a, 0.0, publish=False)
        for i, n in enumerate(rows):
            if n:
                rig.seed(i, *fl.seeded(n, seeds[i]))
        outs = rig.read(b, DT)
        seen = out_bytes(outs)
        for i, (n, o) in enumerate(zip(rows, outs)):
            print("slot %d" % SLOTS_B[i], counts(o))
            assert o["n_tracked_in"] == n and o["n"] > max(n // 2, 512) and o["n_new"] > 0
            if n:
                assert o["n_after_track"] > n // 2 and o["oracle"]["rej"]["hyp"] >= 0
        assert outs[3]["n_new"] == outs[3]["n"]
        # each stream alone, in its slot and in another: the same bytes as inside the batch
        for other in (alone, moved):
            for i, n in enumerate(rows):
                s = other.slots[i]
                other.fr.read_batch([a[i]], 0.0, slots=[s], publish=False)
                if n:
                    other.fr.points_set(*fl.seeded(n, seeds[i]), slot=s)
                assert out_bytes(other.fr.read_batch([b[i]], DT, slots=[s]))[0] == seen[i], (i, s)
    finally:
        for r in (rig, alone, moved):
            r.close()


# ---- c. whole wavefronts in or out -------------------------------------------------------------------------------
def test_a_whole_wavefront_dropped(libs):
    """Rows 64 .. 127, row 0 and row 1023 lie in the border margin: the filter keeps nothing of wavefront 1, and the first and the last
    row of the table go."""
    rig = LimitRig(libs, [6], border=8, equalize=False)
    try:
        out = [0] + list(range(WAVE, 2 * WAVE)) + [CAP - 1]
        pts = fl.strong(CAP)
        pts[out] = fl.margin_points(len(out))
        k = np.arange(CAP)
        rig.read([fl.image(0)], 0.0, publish=False)
        rig.seed(0, pts, fl.ID0 + k, k % 5 + 2)
        o = rig.read([fl.image(1)], DT)[0]
        print(counts(o))
        keep = o["oracle"]["filter"]
        assert o["n_tracked_in"] == CAP and not keep[out].any()
        assert keep.sum() > 512 and keep[1:WAVE].any() and keep[2 * WAVE:3 * WAVE].any() and keep[CAP - WAVE:CAP - 1].any()
        assert o["oracle"]["rej"]["hyp"] >= 0 and o["n"] > 512
    finally:
        rig.close()


def test_one_wavefront_survives(libs):
    """Rows 0 .. 63 are the only ones outside the border margin: the total comes from wavefront 0 alone."""
    rig = LimitRig(libs, [6], border=8, equalize=False)
    try:
        pts = fl.margin_points(CAP)
        pts[:WAVE] = fl.strong(WAVE, margin=24)
        k = np.arange(CAP)
        rig.read([fl.image(0)], 0.0, publish=False)
        rig.seed(0, pts, fl.ID0 + k, k % 5 + 2)
        o = rig.read([fl.image(1)], DT)[0]
        print(counts(o))
        keep = o["oracle"]["filter"]
        assert o["n_tracked_in"] == CAP and not keep[WAVE:].any() and keep[:WAVE].sum() > WAVE // 2
        assert o["n_after_track"] == keep[:WAVE].sum() and o["n"] > 512               # ... and the detection fills the table
    finally:
        rig.close()


# ---- d. more rows than max_cnt -----------------------------------------------------------------------------------
def test_more_rows_than_max_cnt(libs):
    """300 seeded rows under max_cnt = 40 and min_distance = 0: setMask strikes next to nothing, nothing is detected, and the result has
    more rows than max_cnt: the result rows and the lift's grid are sized by the rows the slot holds.  Then max_cnt = 1024."""
    slot = 2
    rig = LimitRig(libs, [slot], max_cnt=40, min_dist=0, equalize=False)
    try:
        rig.read([fl.image(0)], 0.0, publish=False)
        rig.seed(0, *fl.seeded(300))
        o = rig.read([fl.image(1)], DT)[0]
        print(counts(o))
        assert o["n_tracked_in"] == 300 and o["n"] > 256 and o["n_new"] == 0 and o["oracle"]["det"]["n_new"] == 0
        assert len(o["pts"]) == o["n"] and np.all(o["track_cnt"][40:] >= 3) and np.all(np.isfinite(o["un_pts"][40:]))     # (rows past 40 are there)
        got, ft = rig.fr.points_get(slot), rig.fts[0]
        for key, ref in (("pts", ft.cur_pts), ("ids", ft.ids), ("track_cnt", ft.track_cnt), ("prev_un_ids", ft.prev_un_ids),
                         ("prev_un_pts", ft.prev_un_pts)):
            same_bytes(got[key], ref, ("points_get", key))
        assert got["next_id"] == ft.n_id == 0
        rig.set_max_cnt(CAP)
        o2 = rig.read([fl.image(2)], 2 * DT)[0]
        print(counts(o2))
        assert o2["n_tracked_in"] == o["n"] and o2["n_new"] > 0 and o2["n"] > 512 and np.array_equal(o2["ids"][o2["n"] - o2["n_new"]:], np.arange(o2["n_new"]))
    finally:
        rig.close()


# ---- e. two large slots and a small one, repeated ---------------------------------------------------------------
def test_large_and_small_slots_repeat(libs):
    slots, runs, sizes = [0, 8, 3], [], []
    for _ in range(2):
        rig = LimitRig(libs, slots)
        try:
            run = []
            for t in range(4):
                outs = rig.fr.read_batch([fl.image(t, 5), fs.image(64, 48, 7, t), fl.image(t, 6)], DT * t, slots=slots, publish=t != 2)
                run.append(out_bytes(outs))
                sizes.append([o["n"] for o in outs])
            runs.append(run)
        finally:
            rig.close()
    print(sizes[:4])
    assert all(s[0] > 512 and s[2] > 512 and 0 < s[1] < 512 for s in sizes)
    assert runs[0] == runs[1]
    assert all(len({runs[0][t][k] for t in range(4)}) == 4 for k in range(3))           # ... and every frame differs from the others
