"""Predicted pixels in readImage for many streams (include/vio_frame_predict.h; frame.FrameHandle
.set_prediction_batch, .set_prediction_fallback, .read_predict_info; frontend.BatchFeatureTracker.set_predictions) against the per-stream
loop that exists without them: a second handle driven by one FeatureTracker(frames=, rejecter=, slot=s, prediction=) per slot with
set_prediction, followed by update_ids(), fed the same images.  The rigs are those of tests/test_gpu_front.py, test_gpu_front_limits.py
and test_gpu_front_back.py, whose read() holds pts, ids, track_cnt, un_pts, velocity, the counts and feature_frame() to the loop's byte
for byte; here the loop is given the predictions too, and after every read vio_frame_read_predict_info is held to the loop's own
pred_info and to the statuses its tracker calls returned, and vio_frame_points_get (pts, ids, track_cnt, prev_un_ids, prev_un_pts,
next_id) to the loop's tracker (check_info, check_points).  The new path is never the yardstick."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_sequences as fs  # noqa: E402
import front_limits_inputs as fl  # noqa: E402
import test_gpu_front_back as tb  # noqa: E402
from test_gpu_frame import same_bytes  # noqa: E402
from test_gpu_front import DT, Rig, out_bytes  # noqa: E402
from test_gpu_front_cameras import KB_CAM  # noqa: E402
from test_gpu_front_limits import LimitRig  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG = -1
SHIFT = np.float32([1.25, -0.75])                          # a fraction of the 4 x 4 patch: another start, the same basin
FAR = np.float32([-60.0, -60.0])                           # from the left or upper part of a 64 x 48 image: outside it, the point is lost
SPARE = 250                                                # a slot of the oracle handle the rigs do not use
NO_INFO = dict(n_listed=0, n_guessed=0, n_ok_guessed=0, fell_back=False)


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_reject()


@pytest.fixture(scope="module")
def cam_libs(vio, hip_lib):
    return vio, vio.load_frame(), vio.load_camera()


def predict(bt, fts, slots, preds, oracle=True):
    """preds {i: (ids, pixels)} for the next read: to the handle in one call, and (oracle) to the loop's trackers."""
    bt.set_predictions({slots[i]: p for i, p in preds.items()})
    if oracle:
        for i, (ids, px) in preds.items():
            fts[i].set_prediction(ids, px)


def arm(fr, fts, k):
    fr.set_prediction_fallback(k)
    for ft in fts:
        ft.min_tracked = k


def marks(fts):
    return [len(ft.frames.tracks) for ft in fts]


def check_info(fr, slot, ft, listed, before):
    """read_predict_info of the slot's last read against the loop: pred_info, and the tracker calls the loop made in that read (one,
    or two with a fallback; the first is the guessed one)."""
    info = fr.read_predict_info(slot)
    calls = ft.frames.tracks[before:]
    assert info["n_listed"] == listed and info["n_guessed"] == ft.pred_info["n_guessed"] and info["fell_back"] == ft.pred_info["fell_back"], (slot, info, ft.pred_info)
    if listed is not None and info["n_guessed"] + info["n_ok_guessed"] + info["fell_back"] > 0:
        assert len(calls) == (2 if info["fell_back"] else 1), (slot, calls)
    if len(calls) > 0 and ft.pred_info["n_guessed"] > 0:
        assert info["n_ok_guessed"] == calls[0]["ok"], (slot, info, calls)
    check_points(fr, slot, ft)
    return info


def check_points(fr, slot, ft):
    """vio_frame_points_get against the loop's tracker: what the read left resident in the slot, which a published array shows only
    where a further frame follows (after a fallback k_front_take's rows are what the filter, and so this table, was made from)."""
    got = fr.points_get(slot)
    for key, ref in (("pts", ft.cur_pts), ("ids", ft.ids), ("track_cnt", ft.track_cnt), ("prev_un_ids", ft.prev_un_ids), ("prev_un_pts", ft.prev_un_pts)):
        same_bytes(got[key], ref, ("points_get", slot, key))
    assert got["next_id"] == ft.n_id, (slot, got["next_id"], ft.n_id)


def tracks_differ(ofr, slot, cur, guess):
    """On the oracle handle, whose slot still holds the pair: the tracker's positions with the guess are not those without."""
    with_guess, without = ofr.track(cur, guess=guess, slot=slot), ofr.track(cur, slot=slot)
    return with_guess["next_pts"].tobytes() != without["next_pts"].tobytes()


# ---- table sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024])
def test_table_sizes(libs, n):
    slot = 6
    rig = LimitRig(libs, [slot])
    try:
        a, b = fl.image(0), fl.image(1)
        for listing in ("all", "half", "none"):
            rig.reset(0)
            rig.read([a], 0.0, publish=False)
            pts, ids, cnt = fl.seeded(n)
            rig.seed(0, pts, ids, cnt)
            pick = dict(all=np.arange(n), half=np.arange(0, n, 2), none=np.arange(0))[listing]
            pred_ids = ids[pick][::-1] if listing != "none" else np.int64([5, fl.ID0 - 1, fl.ID0 + n, -1])     # descending; or ids no point has
            guess = pts.copy()
            guess[pick] = pts[pick] + SHIFT
            if listing != "none":
                # Row 0, listed either way, is sent out of the image: its guessed track is lost where its own start is not.  The shift
                # alone proves nothing at small n: from a start in the same basin ten Gauss-Newton steps a level end on the same float
                # (observed at n = 1: identical bytes).
                guess[0] = pts[0] + FAR
            pred_px = guess[pick][::-1] if listing != "none" else np.full((4, 2), 7.5, np.float32)
            predict(rig.bt, rig.fts, rig.slots, {0: (pred_ids, pred_px)})
            before = marks(rig.fts)
            o = rig.read([b], fl.DT)[0]
            info = check_info(rig.fr, slot, rig.fts[0], len(pred_ids), before[0])
            print("n %d, %s: %s, after track %d" % (n, listing, info, o["n_after_track"]))
            assert o["n_tracked_in"] == n and info["n_guessed"] == len(pick) and not info["fell_back"]
            assert rig.bt.pred_info == [dict(n_guessed=len(pick), fell_back=False)]
            if listing != "none":
                assert tracks_differ(rig.ofr, slot, pts, guess)           # a prediction that changes nothing proves nothing
                unguessed = rig.ofr.track(pts, slot=slot)["status"]
                assert unguessed[0] == 0 and rig.fts[0].frames.tracks[before[0]]["status"][0] != 0
    finally:
        rig.close()


# ---- one call of six slots ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("publish", [False, True])
def test_six_slots_in_one_call(libs, publish):
    slots, late = [5, 0, 9, 200, 3, 77], 3
    rig = Rig(libs, slots)
    try:
        img = lambda i, t: fs.image(64, 48, 40 + i, t)
        early = [i for i in range(6) if i != late]
        rig.read([img(i, 0) for i in early], 0.0, which=early)
        cur = [rig.fts[i].cur_pts.copy() for i in range(6)]
        ids = [rig.fts[i].ids.copy() for i in range(6)]
        assert all(len(cur[i]) >= 8 for i in early) and len(cur[late]) == 0
        guesses = {}
        for i, k in ((0, np.arange(len(cur[0]))), (1, np.arange(0, len(cur[1]), 2))):
            guesses[i] = cur[i].copy()
            guesses[i][k] = cur[i][k] + SHIFT
            guesses[i][0] = cur[i][0] + FAR                                 # (row 0 is lost for certain: test_table_sizes says why)
        preds = {0: (ids[0], guesses[0]), 1: (ids[1][::2], guesses[1][::2]), 2: (np.zeros(0, np.int64), np.zeros((0, 2), np.float32)),
                 late: (np.arange(5), np.full((5, 2), 20.0, np.float32))}
        predict(rig.bt, rig.fts, slots, preds)
        before = marks(rig.fts)
        outs = rig.read([img(i, 0 if i == late else 1) for i in range(6)], DT, publish=publish)
        infos = [check_info(rig.fr, slots[i], rig.fts[i], len(preds[i][0]) if i in preds else 0, before[i]) for i in range(6)]
        assert infos[0]["n_guessed"] == len(ids[0]) and infos[1]["n_guessed"] == len(ids[1][::2]) and infos[2]["n_guessed"] == 0
        assert infos[late] == dict(NO_INFO, n_listed=5) and infos[4] == NO_INFO and infos[5] == NO_INFO      # one frame: nothing to guess
        assert infos[2]["n_ok_guessed"] == rig.fts[2].frames.tracks[before[2]]["ok"] > 0                     # guessed, with no rows
        assert [p["n_guessed"] for p in rig.bt.pred_info] == [i["n_guessed"] for i in infos]
        assert outs[late]["n_tracked_in"] == 0 and all(outs[i]["n_tracked_in"] == len(cur[i]) for i in early)
        for i in (0, 1):
            assert tracks_differ(rig.ofr, slots[i], cur[i], guesses[i])
        # the frame after, without predictions: one that leaked into a second read would show against the loop
        before = marks(rig.fts)
        rig.read([img(i, 1 if i == late else 2) for i in range(6)], 2 * DT, publish=True)
        assert all(check_info(rig.fr, slots[i], rig.fts[i], 0, before[i]) == NO_INFO for i in range(6))
        assert all(len(rig.fts[i].frames.tracks) == before[i] + 1 for i in early)
    finally:
        rig.close()


# ---- the fallback at its boundary --------------------------------------------------------------------------------
B_SLOTS = [4, 130, 17]


def boundary_rig(libs, back):
    """Three slots after one frame: slot 0 with predictions that send its left and upper points out of the image, slot 1 with good
    ones, slot 2 seeded with three points and no prediction.  Returns the rig, the predictions and the next images."""
    rig = Rig(libs, B_SLOTS)
    if back:
        for h in (rig.fr, rig.ofr):
            h.set_flow_back(levels=2)
        for ft in rig.fts:
            ft.flow_back = dict(levels=2)
    a = [fs.image(64, 48, 50 + i, 0) for i in range(3)]
    rig.read(a, 0.0)
    ft2 = rig.fts[2]
    rig.seed(2, ft2.cur_pts[:3], ft2.ids[:3], ft2.track_cnt[:3])
    cur, ids = rig.fts[0].cur_pts.copy(), rig.fts[0].ids.copy()
    off = (cur[:, 0] < 34) | (cur[:, 1] < 26)
    px0 = np.where(off[:, None], cur + FAR, cur + SHIFT).astype(np.float32)
    px1 = rig.fts[1].cur_pts + SHIFT
    px1[0] = rig.fts[1].cur_pts[0] + FAR                                # (one point lost for certain: the slot's bytes are not an unpredicted read's)
    preds = {0: (ids, px0), 1: (rig.fts[1].ids.copy(), px1)}
    return rig, preds, a, [fs.image(64, 48, 50 + i, 1) for i in range(3)]


def yardstick_ok(rig, i, a, b, pred):
    """The count of status 0 of the loop's guessed call for stream i: FrameHandle.track(guess=) on the oracle handle, a spare slot."""
    ofr, ft = rig.ofr, rig.fts[i]
    ofr.reset(SPARE)
    ofr.push(a, slot=SPARE)
    ofr.push(b, slot=SPARE)
    guess = ft.cur_pts.copy()
    where = {int(d): k for k, d in enumerate(ft.ids)}
    for d, p in zip(*pred):
        guess[where[int(d)]] = p
    n_ok = int((ofr.track(ft.cur_pts, guess=guess, slot=SPARE)["status"] == 0).sum())
    ofr.reset(SPARE)
    return n_ok


@pytest.mark.parametrize("back", [False, True], ids=["check off", "forward-backward check"])
def test_fallback_at_its_boundary(libs, back):
    plain_rig, _, _, b = boundary_rig(libs, back)
    try:
        plain = out_bytes(plain_rig.read(b, DT))                                    # the read without any prediction
    finally:
        plain_rig.close()
    seen = {}
    for step in (0, 1):
        rig, preds, a, b = boundary_rig(libs, back)
        try:
            n = len(rig.fts[0].ids)
            n_ok = yardstick_ok(rig, 0, a[0], b[0], preds[0])
            n_ok1 = yardstick_ok(rig, 1, a[1], b[1], preds[1])
            assert 1 <= n_ok < n and n_ok1 >= n_ok + 1 and n_ok > 3, (n_ok, n, n_ok1)   # or the inputs do not reach the boundary
            arm(rig.fr, rig.fts, n_ok + step)
            predict(rig.bt, rig.fts, B_SLOTS, preds)
            before = marks(rig.fts)
            outs = rig.read(b, DT)
            infos = [check_info(rig.fr, B_SLOTS[i], rig.fts[i], len(preds[i][0]) if i in preds else 0, before[i]) for i in range(3)]
            print("min_tracked %d: %s" % (n_ok + step, infos))
            assert infos[0] == dict(n_listed=n, n_guessed=n, n_ok_guessed=n_ok, fell_back=bool(step))
            assert infos[1]["n_ok_guessed"] == n_ok1 and not infos[1]["fell_back"]
            assert infos[2] == NO_INFO and outs[2]["n_tracked_in"] == 3                 # few points and no guess: it never falls back
            assert [p["fell_back"] for p in rig.bt.pred_info] == [bool(step), False, False]
            if back:
                for i in range(3):
                    assert rig.fr.read_back_info(B_SLOTS[i]) == rig.fts[i].back_info, i
                assert rig.fts[0].back_info["n_checked"] > 0
            seen[step] = out_bytes(outs)
        finally:
            rig.close()
    assert seen[1][0] == plain[0] and seen[0][0] != plain[0]            # fallen back: the bytes of the unpredicted read; guessed: others
    assert seen[0][1] == seen[1][1] != plain[1] and seen[0][2] == seen[1][2] == plain[2]


# ---- a camera of the slot's own ----------------------------------------------------------------------------------
def test_a_slot_with_its_own_camera(cam_libs):
    rig = tb.Rig(cam_libs, [None, KB_CAM, None], flow_back=None)
    try:
        rig.read(0)
        rig.read(1)
        for t, k in ((2, 0), (3, 1024)):                                # a guessed read, then one in which every guessed slot falls back
            arm(rig.fr, rig.fts, k)
            cur = [ft.cur_pts.copy() for ft in rig.fts]
            preds = {i: (ft.ids.copy(), ft.cur_pts + SHIFT) for i, ft in enumerate(rig.fts) if i != 2}
            for p in preds.values():
                p[1][0] += FAR - SHIFT                                  # (row 0 is lost for certain: test_table_sizes says why)
            assert all(len(p[0]) >= 8 for p in preds.values())
            predict(rig.bt, rig.fts, tb.SLOTS, preds)
            before = marks(rig.fts)
            rig.read(t)
            assert all(tracks_differ(rig.ofr, tb.SLOTS[i], cur[i], p[1]) for i, p in preds.items())
            infos = [check_info(rig.fr, tb.SLOTS[i], rig.fts[i], len(preds[i][0]) if i in preds else 0, before[i]) for i in range(3)]
            assert [i["fell_back"] for i in infos] == [k > 0, k > 0, False] and infos[2] == NO_INFO
            assert infos[0]["n_guessed"] > 0 and infos[1]["n_guessed"] > 0 and infos[1]["n_ok_guessed"] > 0
    finally:
        rig.close()


# ---- lifetime ----------------------------------------------------------------------------------------------------
def started(libs, slot=11):
    rig = Rig(libs, [slot])
    rig.read([fs.image(64, 48, 60, 0)], 0.0)
    rig.read([fs.image(64, 48, 60, 1)], DT)
    ft = rig.fts[0]
    assert len(ft.ids) >= 8
    lost = (ft.ids.copy(), ft.cur_pts + FAR)                            # used, it loses every point: nothing like an unpredicted read
    good = (ft.ids[::-1].copy(), ft.cur_pts[::-1] + SHIFT)
    return rig, lost, good


@pytest.mark.parametrize("how", ["clear_prediction", "reset", "push", "set twice", "refused read"])
def test_lifetime(libs, how):
    slot = 11
    rig, lost, good = started(libs, slot)
    try:
        img2, img3 = fs.image(64, 48, 60, 2), fs.image(64, 48, 60, 3)
        predict(rig.bt, rig.fts, rig.slots, {0: lost}, oracle=False)    # pending on the handle alone
        before = marks(rig.fts)
        if how == "clear_prediction":
            rig.fr.clear_prediction(slot)
            rig.fr.clear_prediction(slot)                               # (VIO_OK where there is none)
            o = rig.read([img2], 2 * DT)[0]
            assert o["n_after_track"] > 0 and check_info(rig.fr, slot, rig.fts[0], 0, before[0]) == NO_INFO
        elif how == "reset":
            rig.reset(0)
            assert rig.fr.read_predict_info(slot) == NO_INFO
            rig.read([img2], 2 * DT)
            assert rig.fr.read_predict_info(slot) == NO_INFO            # n_listed 0: the read found no prediction to consume
            before = marks(rig.fts)
            rig.read([img3], 3 * DT)
            assert check_info(rig.fr, slot, rig.fts[0], 0, before[0]) == NO_INFO
        elif how == "push":
            rig.direct_push(0, img2)
            rig.read([img3], 3 * DT)
            assert rig.fr.read_predict_info(slot) == NO_INFO
            check_points(rig.fr, slot, rig.fts[0])
        elif how == "set twice":
            predict(rig.bt, rig.fts, rig.slots, {0: good})              # the second wins, on the handle as in the loop
            o = rig.read([img2], 2 * DT)[0]
            info = check_info(rig.fr, slot, rig.fts[0], len(good[0]), before[0])
            assert info["n_guessed"] == len(good[0]) and o["n_after_track"] > 0
        else:
            rig.fts[0].set_prediction(*lost)
            with pytest.raises(rig.vio.VioError) as e:
                rig.fr.read_batch([img2, img2], 2 * DT, slots=[slot, slot])
            assert e.value.status == BAD_ARG and "twice" in str(e.value)
            o = rig.read([img2], 2 * DT)[0]                             # still pending: this read uses it, as the loop does
            info = check_info(rig.fr, slot, rig.fts[0], len(lost[0]), before[0])
            assert info["n_guessed"] == len(lost[0]) and info["n_ok_guessed"] == 0 and o["n_after_track"] == 0
            before = marks(rig.fts)
            rig.read([img3], 3 * DT)                                    # ... and only this one
            assert check_info(rig.fr, slot, rig.fts[0], 0, before[0]) == NO_INFO
    finally:
        rig.close()


# ---- argument errors ---------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_pending_prediction(libs):
    slot = 11
    rig, lost, good = started(libs, slot)
    try:
        predict(rig.bt, rig.fts, rig.slots, {0: good})
        fr, cap = rig.fr, rig.vio.frame.MAX_TRACK_POINTS
        nan = lost[1].copy()
        nan[3, 1] = np.nan
        inf = lost[1].copy()
        inf[0, 0] = np.inf
        for items, word in (([(slot, np.arange(cap + 1), np.zeros((cap + 1, 2)))], "n must be"), ([(slot, lost[0], nan)], "finite"),
                            ([(slot, lost[0], inf)], "finite"), ([(slot, *lost), (slot + 1, *lost), (slot, *lost)], "twice"),
                            ([(slot + 1, *lost), (rig.vio.frame.MAX_SLOTS, *lost)], "outside"), ([(-1, *lost)], "outside")):
            with pytest.raises(rig.vio.VioError) as e:
                fr.set_prediction_batch(items)
            assert e.value.status == BAD_ARG and word in str(e.value), str(e.value)
        for k in (-1, cap + 1):
            with pytest.raises(rig.vio.VioError) as e:
                fr.set_prediction_fallback(k)
            assert e.value.status == BAD_ARG
        with pytest.raises(rig.vio.VioError):
            fr.clear_prediction(rig.vio.frame.MAX_SLOTS)
        before = marks(rig.fts)
        o = rig.read([fs.image(64, 48, 60, 2)], 2 * DT)[0]             # the earlier prediction is still the one used
        info = check_info(fr, slot, rig.fts[0], len(good[0]), before[0])
        assert info["n_guessed"] == len(good[0]) and o["n_after_track"] > 0
        assert fr.read_predict_info(slot + 1) == NO_INFO               # nothing was stored for the other items of a refused call
        fr.read_batch([fs.image(64, 48, 61, 0)], 0.0, slots=[slot + 1])
        assert fr.read_predict_info(slot + 1) == NO_INFO
    finally:
        rig.close()
