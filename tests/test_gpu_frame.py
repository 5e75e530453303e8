"""The resident-frame library on the GPU (include/vio_frame.h) against the three host-array libraries it shares its kernels with.

The rule everywhere is equality of bytes: a frame's level 0 is ClaheHandle.apply of the image (or the image), its levels above are
FlowHandle.pyramid of that level 0, track is FlowHandle.track on the downloaded pair and detect is DetectHandle.detect on the
downloaded image, in every field.  The same kernels on the same inputs in a fixed order have no tolerance.

The shapes are the smallest at which the new code can go wrong: widths 4k - 1, 4k, 4k + 1 (level 0 has a pitch that is a multiple of 4
where the host-array libraries pack rows tightly), one below, at and above detect's 32 x 8 tile and CLAHE's 128 x 16 block of pixels,
17 x 13 with 8 x 8 CLAHE tiles (a tile size that does not divide), 2 x 5 with one level, and one fixture-sized frame.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as flow_ref  # noqa: E402
from test_frontend_reference import check_frames, fixture_frames  # noqa: E402

pytestmark = pytest.mark.gpu
PREV, NEXT = 0, 1
SHAPES = [(31, 7), (32, 8), (33, 9), (127, 15), (128, 16), (129, 17), (17, 13), (2, 5), (752, 480)]       # (width, height)
SHIFT = (1.3, -0.7)
_cache = {}


def levels_for(w, h, most=4):
    """The most levels (up to `most`) a w x h image has of at least 2 x 2."""
    n = 0
    while n < most and w >= 2 and h >= 2:
        n, w, h = n + 1, w // 2, h // 2
    return n


def images(w, h):
    """Two images of one shape that differ by a small shift (the fixture pair at its size), and a third."""
    key = (w, h)
    if key not in _cache:
        if (w, h) == (752, 480):
            f = fixture_frames()
            _cache[key] = (f[0], f[1], flow_ref.texture(w, h, seed=5))
        else:
            _cache[key] = (flow_ref.texture(w, h, seed=11, smooth=1.5), flow_ref.texture(w, h, seed=11, shift=SHIFT, smooth=1.5),
                           flow_ref.texture(w, h, seed=5, smooth=1.5))
    return _cache[key]


def points(w, h, n=70, seed=2):
    """Keypoints inside the image, then one at the corner (lost: no valid patch), one at the border and a NaN one."""
    rng = np.random.RandomState(seed + w)
    p = np.stack([rng.uniform(0.0, w - 1.0, n), rng.uniform(0.0, h - 1.0, n)], axis=1).astype(np.float32)
    extra = np.array([[0.0, 0.0], [w - 1.2, h / 2.0], [np.nan, 1.0]], dtype=np.float32)
    return np.concatenate([p, extra])


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return vio.load_frame(), vio.load_clahe(), vio.load_flow(), vio.load_detect()


@pytest.fixture(scope="module")
def refs(libs):
    """The three host-array handles the frames are held to."""
    ch, fh, dh = libs[1].create(), libs[2].create(), libs[3].create()
    yield ch, fh, dh
    for h in (ch, fh, dh):
        h.close()


@pytest.fixture()
def fr(libs):
    h = libs[0].create()
    yield h
    h.close()


def same_bytes(a, b, name):
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (name, "%d of %d entries differ" % (int(np.sum(a != b)), a.size))


def same_track(got, ref, name):
    assert sorted(got) == sorted(ref) == ["cost", "iterations", "next_pts", "status"], name
    for k in ("next_pts", "status", "iterations", "cost"):
        same_bytes(got[k], ref[k], (name, k))


def same_detect(got, ref, name):
    assert sorted(got) == sorted(ref), name
    for k in ("status", "n_kept", "n_new", "n_candidates"):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    assert np.float64(got["max_response"]).tobytes() == np.float64(ref["max_response"]).tobytes(), name
    same_bytes(got["keep_order"], ref["keep_order"], (name, "keep_order"))
    same_bytes(got["new_pts"], ref["new_pts"], (name, "new_pts"))


def configure(fr, refs, w, h, equalize=True, inverse=0, half_patch=2, min_distance=3, tiles=(8, 8)):
    ch, fh, dh = refs
    L = levels_for(w, h)
    flow = dict(levels=L, half_patch=half_patch, inverse=inverse)
    fr.set_config(equalize=equalize, clahe=dict(clip_limit=3.0, tiles=tiles), flow=flow, detect=dict(quality=0.01, min_distance=min_distance))
    ch.set_config(clip_limit=3.0, tiles=tiles)
    fh.set_config(**flow)
    dh.set_config(quality=0.01, min_distance=min_distance)
    return L


def level0(refs, img, equalize):
    return refs[0].apply(img) if equalize else np.ascontiguousarray(img)


# ---- push and download ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [True, False])
@pytest.mark.parametrize("w,h", SHAPES)
def test_push_and_download(fr, refs, w, h, equalize):
    a, b, _ = images(w, h)
    wide = np.zeros((h, w + 5), dtype=np.uint8)
    wide[:, :w] = b
    b_strided = wide[:, :w]                                  # rows of another stride than the width
    L = configure(fr, refs, w, h, equalize)
    fr.push(a)
    fr.push(b_strided)
    for which, img in ((PREV, a), (NEXT, b)):
        want0 = level0(refs, img, equalize)
        same_bytes(fr.download(0, which, 0), want0, (w, h, which, 0))
        pyr = refs[1].pyramid(want0)
        assert len(pyr) == L
        for l in range(1, L):
            same_bytes(fr.download(0, which, l), pyr[l], (w, h, which, l))
    if equalize and (w, h) != (2, 5):
        assert fr.download(0, NEXT, 0).tobytes() != b.tobytes()          # (the equalisation did something)


def test_clahe_tiles_and_clip(fr, refs):
    """Other CLAHE settings reach the kernels: 3 x 5 tiles, no clipping."""
    w, h = 129, 17
    a = images(w, h)[0]
    fr.set_config(equalize=True, clahe=dict(clip_limit=0.0, tiles=(3, 5)), flow=dict(levels=1))
    refs[0].set_config(clip_limit=0.0, tiles=(3, 5))
    fr.push(a)
    same_bytes(fr.download(0, NEXT, 0), refs[0].apply(a), "tiles 3 x 5, clip 0")


# ---- track ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("w,h", [(31, 7), (32, 8), (33, 9), (129, 17), (17, 13), (2, 5), (752, 480)])
def test_track_equals_the_flow_library(fr, refs, w, h, inverse):
    a, b, _ = images(w, h)
    configure(fr, refs, w, h, True, inverse, half_patch=4 if w > 100 else 1)
    fr.push(a)
    fr.push(b)
    p0, n0 = fr.download(0, PREV, 0), fr.download(0, NEXT, 0)
    pts = points(w, h)
    guess = (pts + np.float32(0.5)).astype(np.float32)
    for g in (None, guess):
        got, ref = fr.track(pts, guess=g), refs[1].track(p0, n0, pts, guess=g)
        same_track(got, ref, (w, h, inverse, g is not None))
        assert ref["status"][-1] == -3 and np.all(np.isnan(got["next_pts"][-1]))          # the NaN keypoint
        assert ref["status"][-3] == 1                                                     # the corner keypoint is lost
    if (w, h) == (752, 480):
        st = refs[1].track(p0, n0, pts)["status"]
        assert np.sum(st == 0) >= 1 and np.sum(st == 2) + np.sum(st == 1) >= 1           # tracked ones, and lost or border ones


# ---- detect ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("w,h", [(31, 7), (32, 8), (33, 9), (127, 15), (129, 17), (17, 13), (752, 480)])
def test_detect_equals_the_detect_library(fr, refs, w, h, with_mask):
    a = images(w, h)[0]
    big = w > 700
    configure(fr, refs, w, h, True, min_distance=30 if big else 3)
    fr.push(a)
    n0 = fr.download(0, NEXT, 0)
    rng = np.random.RandomState(3)
    tracked = np.stack([rng.uniform(0, w - 1, 12), rng.uniform(0, h - 1, 12)], axis=1).astype(np.float32)
    cnt = rng.randint(1, 5, 12).astype(np.int32)
    mask = None
    if with_mask:
        mask = np.full((h, w), 255, dtype=np.uint8)
        mask[:, : w // 3] = 0
        mask[h // 2, :] = 0
        fr.set_mask(mask)
    first = refs[2].detect(n0, tracked, cnt, mask, 150)
    for max_total in (150, first["n_kept"], max(first["n_kept"] - 1, 0), first["n_kept"] + 1):
        got, ref = fr.detect(tracked, cnt, max_total), refs[2].detect(n0, tracked, cnt, mask, max_total)
        same_detect(got, ref, (w, h, with_mask, max_total))
    same_detect(fr.detect(None, None, 150), refs[2].detect(n0, None, None, mask, 150), (w, h, with_mask, "no tracked points"))
    assert first["n_kept"] >= 1 and (not big or first["n_new"] >= 50)
    if with_mask:
        new = first["new_pts"]
        assert np.all(new[:, 0] >= w // 3) and np.all(new[:, 1] != h // 2)
        fr.set_mask(None)                                                                 # cleared: what it is without one
        same_detect(fr.detect(tracked, cnt, 150), refs[2].detect(n0, tracked, cnt, None, 150), (w, h, "mask cleared"))
    bad = tracked.copy()
    bad[4, 1] = np.inf
    same_detect(fr.detect(bad, cnt, 150), refs[2].detect(n0, bad, cnt, None if with_mask else mask, 150), (w, h, "a non-finite tracked point"))


# ---- slots and rolling ----------------------------------------------------------------------------------------
def test_roll_over_three_pushes(fr, refs, vio):
    w, h = 33, 9
    a, b, c = images(w, h)
    configure(fr, refs, w, h, True)
    ea, eb, ec = (refs[0].apply(x) for x in (a, b, c))
    fr.push(a)
    same_bytes(fr.download(0, NEXT), ea, "first next")
    with pytest.raises(vio.VioError) as e:
        fr.download(0, PREV)
    assert e.value.status == -1 and "too few" in str(e.value)
    fr.push(b)
    same_bytes(fr.download(0, PREV), ea, "second prev")
    same_bytes(fr.download(0, NEXT), eb, "second next")
    fr.push(c)
    same_bytes(fr.download(0, PREV), eb, "third prev")
    same_bytes(fr.download(0, NEXT), ec, "third next")
    fr.push(a)                                               # (the block of the first frame is in use again)
    same_bytes(fr.download(0, PREV), ec, "fourth prev")
    same_bytes(fr.download(0, NEXT), ea, "fourth next")


def track_bytes(o):
    return b"".join(o[k].tobytes() for k in ("next_pts", "status", "iterations", "cost"))


def detect_bytes(o):
    return repr((o["status"], o["n_kept"], o["n_new"], o["n_candidates"])).encode() + np.float64(o["max_response"]).tobytes() + \
        o["keep_order"].tobytes() + o["new_pts"].tobytes()


@pytest.mark.parametrize("inverse", [0, 1])
def test_three_slots_in_one_batch_equal_each_alone(libs, refs, inverse):
    shapes, slots = [(33, 9), (129, 17), (64, 48)], [7, 0, 255]
    flow = dict(levels=2, half_patch=2, inverse=inverse)
    cfg = dict(equalize=True, flow=flow, detect=dict(min_distance=3))
    fr = libs[0].create()
    try:
        fr.set_config(**cfg)
        for k in (0, 1):
            fr.push_batch([dict(slot=s, img=images(w, h)[k]) for s, (w, h) in zip(slots, shapes)])
        titems = [dict(slot=s, prev_pts=points(w, h)) for s, (w, h) in zip(slots, shapes)]
        ditems = [dict(slot=s, tracked=points(w, h)[:9], track_cnt=np.arange(9, dtype=np.int32) % 3 + 1, max_total=40)
                  for s, (w, h) in zip(slots, shapes)]
        tb, db = fr.track_batch(titems), fr.detect_batch(ditems)
        # a repeat equals itself
        assert [track_bytes(o) for o in fr.track_batch(titems)] == [track_bytes(o) for o in tb]
        assert [detect_bytes(o) for o in fr.detect_batch(ditems)] == [detect_bytes(o) for o in db]
        levels0 = [fr.download(s, NEXT, 0) for s in slots]
    finally:
        fr.close()
    for i, (w, h) in enumerate(shapes):                      # each alone, on a handle of its own, in another slot
        one = libs[0].create()
        try:
            one.set_config(**cfg)
            one.push(images(w, h)[0], slot=3)
            one.push(images(w, h)[1], slot=3)
            assert track_bytes(one.track(titems[i]["prev_pts"], slot=3)) == track_bytes(tb[i]), (w, h)
            assert detect_bytes(one.detect(ditems[i]["tracked"], ditems[i]["track_cnt"], 40, slot=3)) == detect_bytes(db[i]), (w, h)
            same_bytes(one.download(3, NEXT, 0), levels0[i], (w, h))
        finally:
            one.close()
        assert db[i]["n_kept"] >= 1
    assert sum(int(np.sum(o["status"] == 0)) for o in tb) >= 1


def test_reset_accepts_a_new_geometry(fr, refs, vio):
    configure(fr, refs, 33, 9, True)
    a, b, _ = images(33, 9)
    fr.push(a)
    fr.push(b)
    before = fr.counters()
    other = images(32, 8)[0]
    with pytest.raises(vio.VioError) as e:
        fr.push(other)
    assert e.value.status == -1 and "item 0" in str(e.value) and "reset" in str(e.value)
    assert fr.counters() == before                           # nothing was uploaded ...
    same_bytes(fr.download(0, PREV), refs[0].apply(a), "prev after the refused push")         # ... or rolled
    same_bytes(fr.download(0, NEXT), refs[0].apply(b), "next after the refused push")
    fr.reset(0)
    with pytest.raises(vio.VioError):
        fr.track(points(33, 9))
    fr.push(other)
    same_bytes(fr.download(0, NEXT), refs[0].apply(other), "the new geometry")
    # a change of levels drops the frames too
    fr.push(other)
    fr.set_config(flow=dict(levels=1))
    with pytest.raises(vio.VioError) as e:
        fr.detect(None, None, 10)
    assert e.value.status == -1


# ---- counters -------------------------------------------------------------------------------------------------
def test_counters(fr, refs):
    w, h = 33, 9
    a, b, c = images(w, h)
    configure(fr, refs, w, h, True)
    assert fr.counters() == dict(image_up=0, image_down=0, other_up=0, other_down=0)
    for k, img in enumerate((a, b, c, a, b)):
        fr.push(img)
        assert fr.counters()["image_up"] == (k + 1) * w * h
    c0 = fr.counters()
    assert c0["image_down"] == 0 and c0["other_down"] == 0 and c0["other_up"] > 0
    fr.track(points(w, h))
    fr.detect(points(w, h)[:5], None, 20)
    c1 = fr.counters()
    assert (c1["image_up"], c1["image_down"]) == (5 * w * h, 0)           # tracking and detecting move no image
    assert c1["other_up"] > c0["other_up"] and c1["other_down"] > 0
    fr.download(0, NEXT, 0)
    c2 = fr.counters()
    assert (c2["image_up"], c2["image_down"], c2["other_down"]) == (5 * w * h, w * h, c1["other_down"])
    fr.download(0, PREV, 1)                                                  # a level above 0 is not image bytes
    c3 = fr.counters()
    assert c3["image_down"] == w * h and c3["other_down"] == c2["other_down"] + (w // 2) * (h // 2)
    fr.set_mask(np.full((h, w), 255, dtype=np.uint8))                        # a mask is
    assert fr.counters()["image_up"] == 6 * w * h
    t = fr.timing()
    assert all(np.isfinite(t[k]) and t[k] >= 0.0 for k in t), t


# ---- bad arguments --------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(fr, refs, vio):
    from vio_amd import frame
    w, h = 33, 9
    a, b, _ = images(w, h)
    configure(fr, refs, w, h, True)
    fr.push(a, slot=1)
    fr.push(b, slot=1)
    fr.push(a, slot=2)                                       # one frame only
    kept = [fr.download(1, PREV).copy(), fr.download(1, NEXT).copy(), fr.download(2, NEXT).copy()]
    before = fr.counters()

    def refused(call, *words):
        with pytest.raises(vio.VioError) as e:
            call()
        assert e.value.status == -1, e.value
        for wd in words:
            assert wd in str(e.value), (wd, str(e.value))

    pts = points(w, h)
    refused(lambda: fr.push(a, slot=frame.MAX_SLOTS), "item 0", "outside")
    refused(lambda: fr.push(a, slot=-1), "outside")
    refused(lambda: fr.push_batch([dict(slot=4, img=a), dict(slot=1, img=a), dict(slot=4, img=a)]), "item 2", "twice")
    refused(lambda: fr.push_batch([dict(slot=4, img=a), dict(slot=1, img=images(32, 8)[0])]), "item 1", "reset")
    refused(lambda: fr.push(np.zeros((2, frame.MAX_DIM + 1), dtype=np.uint8), slot=5), "item 0")
    refused(lambda: fr.push(np.zeros((4, 4), dtype=np.uint8), slot=5), "2 x 2")           # the three levels of 4 x 4 end at 1 x 1
    refused(lambda: fr.push_batch([dict(slot=s % frame.MAX_SLOTS, img=a) for s in range(frame.MAX_SLOTS + 1)]), "count")
    refused(lambda: fr.track(pts, slot=2), "item 0", "too few")                             # one frame
    refused(lambda: fr.track(pts, slot=3), "too few")                                       # none
    refused(lambda: fr.track(pts, slot=frame.MAX_SLOTS), "outside")
    refused(lambda: fr.track_batch([dict(slot=1, prev_pts=pts), dict(slot=1, prev_pts=np.zeros((4097, 2), dtype=np.float32))]), "item 1", "n_pts")
    refused(lambda: fr.detect(None, None, 10, slot=3), "item 0", "too few")                 # no frame
    refused(lambda: fr.detect(None, None, 4097, slot=1), "item 0")
    refused(lambda: fr.detect(np.array([[w + 3.0, 1.0]], dtype=np.float32), None, 10, slot=1), "outside")
    refused(lambda: fr.detect(None, None, 10, slot=-2), "outside")
    refused(lambda: fr.set_mask(np.ones((h, w), dtype=np.uint8), slot=frame.MAX_SLOTS), "outside")
    refused(lambda: fr.reset(frame.MAX_SLOTS), "outside")
    fr.shapes[9] = (h, w)
    refused(lambda: fr.download(9, NEXT, 0), "too few")
    refused(lambda: fr.download(1, 2, 0))
    fr.shapes.pop(9)
    # a mask of another geometry makes the slot's detection an error until it is replaced or cleared
    fr.set_mask(np.ones((h, w + 1), dtype=np.uint8), slot=1)
    refused(lambda: fr.detect(None, None, 10, slot=1), "mask")
    fr.set_mask(None, slot=1)
    after_mask = dict(before, image_up=before["image_up"] + h * (w + 1))
    assert fr.counters() == after_mask
    # the raw call: a bad second item leaves the output arrays as they were
    items = (frame.VioFrameTrackItem * 2)()
    p = np.ascontiguousarray(pts[:4])
    items[0] = frame.VioFrameTrackItem(1, 4, p.ctypes.data, None)
    items[1] = frame.VioFrameTrackItem(2, 4, p.ctypes.data, None)
    out = np.full((8, 2), 7.5, dtype=np.float32)
    info = (frame.VioFlowPtInfo * 8)()
    C.memset(info, 0x5A, C.sizeof(info))
    assert fr.lib.fn["track_batch"](fr.h, 2, C.addressof(items), out.ctypes.data, C.addressof(info)) == -1
    assert np.all(out == 7.5) and bytes(info) == b"\x5a" * C.sizeof(info)
    assert b"item 1" in fr.lib.fn["last_error"](fr.h)
    assert fr.lib.fn["push_batch"](fr.h, 1, None) == -1 and fr.lib.fn["push_batch"](fr.h, -1, None) == -1
    assert fr.lib.fn["push_batch"](fr.h, 0, None) == 0
    with pytest.raises(vio.VioError):
        fr.set_config(flow=dict(levels=9))
    with pytest.raises(vio.VioError):
        fr.set_config(clahe=dict(tiles=(17, 8)))
    with pytest.raises(vio.VioError):
        fr.set_config(detect=dict(quality=0.0))
    # nothing moved and nothing rolled
    assert fr.counters() == after_mask
    for got, want, name in zip([fr.download(1, PREV), fr.download(1, NEXT), fr.download(2, NEXT)], kept, ("1 prev", "1 next", "2 next")):
        same_bytes(got, want, name)
    same_track(fr.track(pts, slot=1), refs[1].track(kept[0], kept[1], pts), "slot 1 still tracks")


# ---- the front end --------------------------------------------------------------------------------------------
def test_front_end_equals_the_three_handles(vio, libs, refs):
    frames = fixture_frames()
    ch, fh, dh = refs
    ch.set_config()
    fh.set_config()
    fr = libs[0].create()
    try:
        fr.set_config(equalize=True)
        resident = vio.FeatureTracker(None, None, max_cnt=150, min_dist=30, frames=fr, slot=1)
        outs = check_frames(resident, frames)
        hosted = vio.FeatureTracker(fh, dh, max_cnt=150, min_dist=30, equalizer=ch)
        want = check_frames(hosted, frames)
        for t, (o, r) in enumerate(zip(outs, want)):
            assert o["n_new"] == r["n_new"], t
            for k in ("pts", "ids", "track_cnt"):
                same_bytes(o[k], r[k], (t, k))
        assert np.sum(outs[2]["track_cnt"] == 3) >= 1                                    # (points were tracked through all three)
        hh, ww = frames[0].shape
        c = fr.counters()
        assert c["image_up"] == 3 * ww * hh and c["image_down"] == 0
        assert resident.cur_img is None and resident.prev_img is None
        same_bytes(fr.download(1, NEXT), hosted.cur_img, "cur_img")
        same_bytes(fr.download(1, PREV), hosted.prev_img, "prev_img")
    finally:
        fr.close()
