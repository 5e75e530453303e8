"""The resident-frame library (include/vio_frame.h) over sequences of calls: what it keeps on the device between calls.

tests/test_gpu_frame.py holds one fresh handle and one geometry per case.  Here a handle lives through many calls: blocks handed on to
another geometry, another slot or a mask (the pool's contents are stale, never cleared), staging and table buffers regrown under a
push that nothing has waited for, settings that change between two pushes of a slot, full batches of 256 items, eight pyramid levels,
the caller's stream.  The rule is that of tests/test_gpu_frame.py, equality of bytes with no tolerance, and so is the oracle: level 0
is ClaheHandle.apply of the pushed image (or the image), the levels above are FlowHandle.pyramid of it, track is FlowHandle.track on the
model's pair, detect is DetectHandle.detect on the model's next with the model's mask.  The sequences are those of
tests/frame_sequences.py with the seeds tests/test_frame_sequences_cpu.py holds to what they must reach.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as flow_ref  # noqa: E402
import frame_sequences as fs  # noqa: E402
from test_frame_sequences_cpu import N_OPS, SEEDS  # noqa: E402
from test_gpu_flow import compare, grid_pts, pair  # noqa: E402
from test_gpu_frame import (NEXT, PREV, detect_bytes, images, libs, points, refs, same_bytes, same_detect, same_track,  # noqa: E402,F401
                            track_bytes)

pytestmark = pytest.mark.gpu


class HandleOracle:
    """The three host-array handles behind the interface frame_sequences.run() asks of an oracle."""

    def __init__(self, refs):  # noqa: F811
        self.ch, self.fh, self.dh = refs

    def apply(self, img, clip_limit=3.0, tiles=(8, 8)):
        self.ch.set_config(clip_limit=clip_limit, tiles=tiles)
        return self.ch.apply(np.ascontiguousarray(img))

    def pyramid(self, level0, levels):
        self.fh.set_config(levels=levels)
        return self.fh.pyramid(level0)

    def track(self, prev0, next0, pts, guess, levels, half_patch, inverse):
        self.fh.set_config(levels=levels, half_patch=half_patch, inverse=inverse)
        return self.fh.track(prev0, next0, pts, guess)

    def detect(self, img, tracked, track_cnt, mask, max_total, quality=0.01, min_distance=3):
        self.dh.set_config(quality=quality, min_distance=min_distance)
        return self.dh.detect(img, tracked, track_cnt, mask, max_total)


@pytest.fixture(scope="module")
def oracle(refs):  # noqa: F811
    return HandleOracle(refs)


@pytest.fixture()
def make(libs):  # noqa: F811
    """make(**create's arguments): a frame handle that is closed after the test."""
    made = []

    def one(**kw):
        made.append(libs[0].create(**kw))
        return made[-1]
    yield one
    for h in made:
        h.close()


def config(fr, equalize=True, tiles=(8, 8), levels=2, half_patch=2, inverse=0, min_distance=3):
    fr.set_config(equalize=equalize, clahe=dict(clip_limit=3.0, tiles=tiles), flow=dict(levels=levels, half_patch=half_patch, inverse=inverse),
                  detect=dict(quality=0.01, min_distance=min_distance))
    return dict(equalize=equalize, tiles=tiles, levels=levels, half_patch=half_patch, inverse=inverse, min_distance=min_distance)


def level0(oracle, img, cfg):
    return oracle.apply(img, 3.0, cfg["tiles"]) if cfg["equalize"] else np.ascontiguousarray(img)


def detect_item(w, h, slot, n=9, max_total=40):
    return dict(slot=slot, tracked=points(w, h)[:n], track_cnt=np.arange(n, dtype=np.int32) % 3 + 1, max_total=max_total)


def check_slots(fr, oracle, cfg, want, name, masks=None, n_pts=70):
    """want: slot -> (level 0 of prev, level 0 of next).  Every level of both by download, then one track_batch and one detect_batch
    over all the slots, against the oracle.  Returns the bytes of everything the handle gave."""
    masks, out = masks or {}, []
    for s, pair0 in sorted(want.items()):
        for which, l0 in zip((PREV, NEXT), pair0):
            pyr = oracle.pyramid(l0, cfg["levels"])
            for l in range(cfg["levels"]):
                got = fr.download(s, which, l)
                same_bytes(got, pyr[l], (name, "slot", s, "which", which, "level", l))
                out.append(got.tobytes())
    slots = sorted(want)
    titems = [dict(slot=s, prev_pts=points(want[s][1].shape[1], want[s][1].shape[0], n=n_pts)) for s in slots]
    for s, it, got in zip(slots, titems, fr.track_batch(titems)):
        same_track(got, oracle.track(want[s][0], want[s][1], it["prev_pts"], None, cfg["levels"], cfg["half_patch"], cfg["inverse"]),
                   (name, "track", s))
        out.append(track_bytes(got))
    ditems = [detect_item(want[s][1].shape[1], want[s][1].shape[0], s) for s in slots]
    for s, it, got in zip(slots, ditems, fr.detect_batch(ditems)):
        same_detect(got, oracle.detect(want[s][1], it["tracked"], it["track_cnt"], masks.get(s), it["max_total"], 0.01, cfg["min_distance"]),
                    (name, "detect", s))
        out.append(detect_bytes(got))
    return out


# ---- random sequences -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences(make, oracle, seed):
    seq = fs.make_sequence(seed, N_OPS)
    first = fs.run(seq, make(), oracle)
    again = fs.run(seq, make(), oracle)                      # another handle, the same calls: the same bytes
    assert len(first) >= 20 and [n for n, _ in first] == [n for n, _ in again]
    for (name, a), (_, b) in zip(first, again):
        assert a == b, name


# ---- a block that held something else -------------------------------------------------------------------------
def test_reuse_of_a_block_by_another_geometry(make, oracle):
    """At 2 levels a 64 x 48 frame is 3840 bytes, a 64 x 48 mask 3072, a 61 x 45 frame 3840, a 129 x 17 frame 2816.  Slot 0's three pushes
    leave the blocks b0, b1, b2 (b0 free); the mask takes b0; after the reset the 61 x 45 frame takes b1 (a block of its size that held
    another geometry), the first 129 x 17 frame b2 (a larger block), and once the mask is cleared the second 129 x 17 frame b0 (a
    block that held a mask).  tests/test_frame_sequences_cpu.py counts the same hand-overs in the random sequences."""
    A, B, Cc = (64, 48), (61, 45), (129, 17)
    fr = make()
    cfg = config(fr, equalize=True, levels=2)
    for k in (0, 1, 2):
        fr.push(images(*A)[k], slot=0)
    fr.set_mask(fs.mask_image(64, 48, 0), slot=1)
    fr.reset(0)
    fr.push_batch([dict(slot=0, img=images(*B)[0]), dict(slot=2, img=images(*Cc)[0])])
    fr.set_mask(None, slot=1)
    fr.push(images(*Cc)[2], slot=3)
    fr.push_batch([dict(slot=0, img=images(*B)[1]), dict(slot=2, img=images(*Cc)[1]), dict(slot=3, img=images(*Cc)[0])])
    final = {0: (images(*B)[0], images(*B)[1]), 2: (images(*Cc)[0], images(*Cc)[1]), 3: (images(*Cc)[2], images(*Cc)[0])}
    want = {s: tuple(level0(oracle, im, cfg) for im in p) for s, p in final.items()}
    got = check_slots(fr, oracle, cfg, want, "reused blocks")
    fresh = make()                                           # a handle that was only ever given the final two frames of each slot
    config(fresh, equalize=True, levels=2)
    for k in (0, 1):
        fresh.push_batch([dict(slot=s, img=final[s][k]) for s in sorted(final)])
    assert got == check_slots(fresh, oracle, cfg, want, "fresh blocks")


# ---- regrowth under a push nothing has waited for ---------------------------------------------------------------
@pytest.mark.parametrize("equalize", [True, False])
def test_back_to_back_pushes_that_grow_the_buffers(make, oracle, equalize):
    """One small push, then a batch whose staging, tables and look-up tables are all larger, a mask, and all nine again, with nothing
    between them that waits for the device: the first push's kernels may still be running when its buffers are released."""
    small, big = images(33, 9), images(129, 17)
    a = {0: small[0]}
    b = {0: small[1]}
    for s in range(1, 9):
        a[s], b[s] = np.roll(big[0], s, axis=0), np.roll(big[1], s, axis=0)
    mask = fs.mask_image(129, 17, 1)
    fr = make()
    cfg = config(fr, equalize=equalize, levels=2)
    fr.push(a[0], slot=0)
    fr.push_batch([dict(slot=s, img=a[s]) for s in range(1, 9)])
    fr.set_mask(mask, slot=3)
    fr.push_batch([dict(slot=s, img=b[s]) for s in range(9)])
    want = {s: (level0(oracle, a[s], cfg), level0(oracle, b[s], cfg)) for s in range(9)}
    check_slots(fr, oracle, cfg, want, "grown buffers, equalize %d" % equalize, masks={3: np.ascontiguousarray(mask)})


# ---- the most items a call may have ---------------------------------------------------------------------------
def test_256_slots_in_one_call(make, refs):  # noqa: F811
    from vio_amd import frame
    ch, fh, dh = refs
    w, h, n = 16, 12, frame.MAX_SLOTS
    base = [flow_ref.texture(w, h, seed=11, smooth=1.5), flow_ref.texture(w, h, seed=11, shift=(0.6, -0.4), smooth=1.5)]
    imgs = [[np.roll(base[k], s, axis=0) for s in range(n)] for k in (0, 1)]
    fr = make()
    cfg = config(fr, equalize=True, levels=2, half_patch=1)
    for k in (0, 1):
        fr.push_batch([dict(slot=s, img=imgs[k][s]) for s in range(n)])
    ch.set_config(clip_limit=3.0, tiles=(8, 8))
    l0 = [ch.apply_batch(imgs[k]) for k in (0, 1)]
    for s in range(n):
        for k in (0, 1):
            same_bytes(fr.download(s, k, 0), l0[k][s], ("level 0", s, k))
    empty = (3, 128, 255)                                    # items without keypoints, and without room for a corner
    none = np.zeros((0, 2), dtype=np.float32)
    pts = points(w, h, n=10)
    titems = [dict(slot=s, prev_pts=none if s in empty else pts) for s in range(n)]
    fh.set_config(levels=2, half_patch=1)
    tb = fr.track_batch(titems)
    ref = fh.track_batch([dict(img_prev=l0[0][s], img_next=l0[1][s], prev_pts=titems[s]["prev_pts"]) for s in range(n)])
    for s in range(n):
        same_track(tb[s], ref[s], ("track", s))
        assert len(tb[s]["status"]) == (0 if s in empty else len(pts))
    assert sum(int(np.sum(o["status"] == 0)) for o in tb) >= n
    ditems = [dict(slot=s, tracked=None, track_cnt=None, max_total=0) if s in empty else detect_item(w, h, s, n=5, max_total=12) for s in range(n)]
    dh.set_config(quality=0.01, min_distance=3)
    db = fr.detect_batch(ditems)
    ref = dh.detect_batch([dict(img=l0[1][s], tracked=ditems[s]["tracked"], track_cnt=ditems[s]["track_cnt"], max_total=ditems[s]["max_total"])
                           for s in range(n)])
    for s in range(n):
        same_detect(db[s], ref[s], ("detect", s))
        assert db[s]["n_new"] == 0 if s in empty else db[s]["n_kept"] >= 1
    assert sum(o["n_new"] for o in db) >= n
    # the last and the first slot against the same frames alone in slot 7 of another handle
    one = make()
    config(one, equalize=True, levels=2, half_patch=1)
    for s in (n - 1, 0):
        one.reset(7)
        for k in (0, 1):
            one.push(imgs[k][s], slot=7)
        for k in (0, 1):
            for l in (0, 1):
                same_bytes(one.download(7, k, l), fr.download(s, k, l), ("alone", s, k, l))
        if s not in empty:
            assert track_bytes(one.track(pts, slot=7)) == track_bytes(tb[s])
            assert detect_bytes(one.detect(ditems[s]["tracked"], ditems[s]["track_cnt"], 12, slot=7)) == detect_bytes(db[s])
        else:
            assert detect_bytes(one.detect(None, None, 0, slot=7)) == detect_bytes(db[s])
    # a call whose every item is empty: OK, and the output arrays are as they were
    items = (frame.VioFrameTrackItem * n)()
    for s in range(n):
        items[s] = frame.VioFrameTrackItem(s, 0, None, None)
    out = np.full((8, 2), 7.5, dtype=np.float32)
    info = (frame.VioFlowPtInfo * 8)()
    C.memset(info, 0x5A, C.sizeof(info))
    assert fr.lib.fn["track_batch"](fr.h, n, C.addressof(items), out.ctypes.data, C.addressof(info)) == 0
    assert np.all(out == 7.5) and bytes(info) == b"\x5a" * C.sizeof(info)


# ---- level 0 written by per-item copies -----------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(31, 7), (33, 9), (129, 17)])
def test_equalize_off_tracks_and_detects(make, oracle, w, h):
    a, b, _ = images(w, h)
    fr = make()
    pts = points(w, h)
    guess = (pts + np.float32(0.5)).astype(np.float32)
    tracked, cnt = points(w, h)[:9], np.arange(9, dtype=np.int32) % 3 + 1
    mask = fs.mask_image(w, h, 1)
    for inverse in (0, 1):
        cfg = config(fr, equalize=False, levels=2 if h > 7 else 1, half_patch=4 if w > 100 else 1, inverse=inverse)
        fr.push(a)
        fr.push(b)
        same_bytes(fr.download(0, PREV, 0), a, (w, h, "prev is the image"))
        same_bytes(fr.download(0, NEXT, 0), b, (w, h, "next is the image"))
        for g in (None, guess):
            same_track(fr.track(pts, guess=g), oracle.track(a, b, pts, g, cfg["levels"], cfg["half_patch"], inverse), (w, h, inverse, g is not None))
        for m in (None, mask):
            fr.set_mask(m)
            ref = oracle.detect(b, tracked, cnt, None if m is None else np.ascontiguousarray(m), 40)
            same_detect(fr.detect(tracked, cnt, 40), ref, (w, h, inverse, m is not None))
            assert ref["n_kept"] >= 1
        fr.set_mask(None)


# ---- the library's own copy of k_clahe_apply at the largest tile grid ------------------------------------------
@pytest.mark.parametrize("tiles", [(16, 16), (1, 1)])
@pytest.mark.parametrize("w,h", [(129, 17), (64, 48)])
def test_clahe_tile_grids_on_the_resident_path(make, oracle, w, h, tiles):
    a, b, _ = images(w, h)
    fr = make()
    cfg = config(fr, equalize=True, tiles=tiles, levels=2)
    fr.push_batch([dict(slot=0, img=a), dict(slot=9, img=b)])
    for s, img in ((0, a), (9, b)):
        want = oracle.apply(img, 3.0, tiles)
        pyr = oracle.pyramid(want, 2)
        for l in (0, 1):
            same_bytes(fr.download(s, NEXT, l), pyr[l], (w, h, tiles, s, l))
        assert want.tobytes() != img.tobytes()
    assert cfg["tiles"] == tiles and oracle.apply(a, 3.0, tiles).tobytes() != oracle.apply(a, 3.0, (8, 8)).tobytes()


# ---- prev keeps the settings it was pushed under ---------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
def test_settings_change_between_two_pushes(make, oracle, inverse):
    w, h = 129, 17
    a, b, c = images(w, h)
    fr = make()
    pts = points(w, h)
    steps = [(a, dict(equalize=True, tiles=(8, 8))), (b, dict(equalize=True, tiles=(3, 5))), (c, dict(equalize=False, tiles=(3, 5)))]
    prev = None
    for k, (img, kw) in enumerate(steps):
        cfg = config(fr, levels=2, half_patch=4, inverse=inverse, **kw)
        fr.push(img)
        cur = level0(oracle, img, cfg)
        same_bytes(fr.download(0, NEXT, 0), cur, (k, "next under the current settings"))
        same_bytes(fr.download(0, NEXT, 1), oracle.pyramid(cur, 2)[1], (k, "next, level 1"))
        if prev is not None:
            same_bytes(fr.download(0, PREV, 0), prev, (k, "prev under the earlier settings"))
            same_bytes(fr.download(0, PREV, 1), oracle.pyramid(prev, 2)[1], (k, "prev, level 1"))
            same_track(fr.track(pts), oracle.track(prev, cur, pts, None, 2, 4, inverse), (k, "track over the change"))
            assert prev.tobytes() != level0(oracle, steps[k - 1][0], cfg).tobytes()          # (the settings do differ in their bytes)
        prev = cur


# ---- masks ----------------------------------------------------------------------------------------------------
def test_masks(make, oracle):
    w, h = 33, 9
    a, b, _ = images(w, h)
    fr = make()
    cfg = config(fr, equalize=True, levels=2)
    masks = {s: fs.mask_image(w, h, s) for s in (0, 1, 2)}
    assert masks[1].strides[0] > w and masks[1].base[0, w] == 255          # strided rows, the padding open
    flat = {s: np.ascontiguousarray(m) for s, m in masks.items()}
    fr.set_mask(masks[2], slot=2)                             # before the slot's first push
    fr.push_batch([dict(slot=s, img=a) for s in (0, 1, 2)])
    fr.set_mask(masks[0], slot=0)
    fr.set_mask(masks[1], slot=1)
    n0 = level0(oracle, a, cfg)
    items = [detect_item(w, h, s) for s in (0, 1, 2)]

    def ref(m):
        return oracle.detect(n0, items[0]["tracked"], items[0]["track_cnt"], m, 40)
    outs = fr.detect_batch(items)
    for s in (0, 1, 2):
        same_detect(outs[s], ref(flat[s]), ("three masks", s))
    assert len({detect_bytes(o) for o in outs}) == 3 and detect_bytes(outs[0]) != detect_bytes(ref(None))
    # another mask of the same size on slot 1 (it takes another block: the old one is released after the new one is taken)
    fr.set_mask(masks[2], slot=1)
    outs2 = fr.detect_batch(items)
    same_detect(outs2[1], ref(flat[2]), "replaced")
    assert detect_bytes(outs2[0]) == detect_bytes(outs[0]) and detect_bytes(outs2[2]) == detect_bytes(outs[2])
    # the mask outlives a reset and a push of the same geometry ...
    fr.reset(0)
    fr.push(b, slot=0)
    same_detect(fr.detect(items[0]["tracked"], items[0]["track_cnt"], 40, slot=0),
                oracle.detect(level0(oracle, b, cfg), items[0]["tracked"], items[0]["track_cnt"], flat[0], 40), "after a reset")
    # ... and a change of levels, which drops the frames
    cfg = config(fr, equalize=True, levels=1)
    fr.push_batch([dict(slot=s, img=b) for s in (0, 1, 2)])
    n1 = level0(oracle, b, cfg)
    for s, m, o in zip((0, 1, 2), (flat[0], flat[2], flat[2]), fr.detect_batch(items)):
        same_detect(o, oracle.detect(n1, items[0]["tracked"], items[0]["track_cnt"], m, 40), ("after a change of levels", s))


# ---- pyramid levels 5 to 8 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("levels", [5, 8])
@pytest.mark.parametrize("w,h", [(256, 256), (259, 257)])
def test_levels_5_to_8(make, refs, w, h, levels, inverse):  # noqa: F811
    """256 x 256 is the smallest image with eight levels of at least 2 x 2.  The flow library against the numpy restatement under the
    rule of tests/test_gpu_flow.py, then the frame library against the flow library in every byte."""
    fh = refs[1]
    a, b = pair(w, h)
    pts = grid_pts(w, h, 24, 12)
    fr = make()
    for half_patch in (4, 1):
        fh.set_config(levels=levels, half_patch=half_patch, inverse=inverse)
        pyr = fh.pyramid(a)
        want = flow_ref.pyramid(a, levels)
        assert len(pyr) == levels and pyr[-1].shape == (h >> (levels - 1), w >> (levels - 1))
        for g, r in zip(pyr, want):
            assert g.shape == r.shape and np.array_equal(g, r)
        ref = flow_ref.multi_level(a, b, pts, levels=levels, half_patch=half_patch, inverse=inverse, order="wave64")
        # the restatement tracks all 24 with the 8 x 8 patch.  With the 2 x 2 patch it loses up to 15 of them on every image tried
        # (smooth and fine textures, noise moved by a whole pixel): the coarse levels, down to 2 x 2 pixels, throw keypoints out of
        # the image.  Those cases hold tracked and lost keypoints alike to the restatement.
        assert np.all(ref[1] == flow_ref.OK) if half_patch == 4 else np.any(ref[1] == flow_ref.OK), ref[1]
        got = fh.track(a, b, pts)
        compare(got, ref, "%dx%d L%d h%d inv%d" % (w, h, levels, half_patch, inverse))
        config(fr, equalize=False, levels=levels, half_patch=half_patch, inverse=inverse)
        fr.push(a)
        fr.push(b)
        for l in range(levels):
            same_bytes(fr.download(0, PREV, l), pyr[l], (w, h, levels, "level", l))
        same_track(fr.track(pts), got, (w, h, levels, half_patch, inverse))


# ---- the caller's stream and device ---------------------------------------------------------------------------
def test_callers_stream_and_device(make, oracle):
    import torch
    w, h = 129, 17
    a, b, _ = images(w, h)
    stream = torch.cuda.Stream()
    cur = torch.cuda.current_device()
    outs = []
    for kw in (dict(stream=stream.cuda_stream), dict()):
        fr = make(**kw)
        got = []
        for call in (lambda: config(fr, equalize=True, levels=2), lambda: fr.push(a), lambda: fr.push(b),
                     lambda: fr.set_mask(fs.mask_image(w, h, 0)),
                     lambda: got.append(track_bytes(fr.track(points(w, h)))),
                     lambda: got.append(detect_bytes(fr.detect(points(w, h)[:9], None, 40))),
                     lambda: got.extend(fr.download(0, which, l).tobytes() for which in (PREV, NEXT) for l in (0, 1)),
                     lambda: fr.reset(0), lambda: fr.counters(), lambda: fr.timing()):
            call()
            assert torch.cuda.current_device() == cur
        outs.append(got)
        fr.close()
        assert torch.cuda.current_device() == cur
    assert outs[0] == outs[1] and len(outs[0]) == 6
    cfg = dict(equalize=True, tiles=(8, 8), levels=2)
    assert outs[0][2] == level0(oracle, a, cfg).tobytes() and outs[0][4] == level0(oracle, b, cfg).tobytes()
    stream.synchronize()


# ---- the largest point counts ---------------------------------------------------------------------------------
def test_largest_point_counts(make, oracle):
    from vio_amd import flow
    w, h = 64, 48
    a, b, _ = images(w, h)
    fr = make()
    cfg = config(fr, equalize=True, levels=2, min_distance=0)
    fr.push_batch([dict(slot=0, img=a), dict(slot=1, img=a)])
    fr.push_batch([dict(slot=0, img=b), dict(slot=1, img=b)])
    p0, n0 = level0(oracle, a, cfg), level0(oracle, b, cfg)
    many = points(w, h, n=flow.MAX_POINTS - 3)                # 4096 with the lost, the border and the NaN keypoint
    assert len(many) == flow.MAX_POINTS == 4096
    tracked = np.ascontiguousarray(many[:-1][np.arange(4096) % 4095])                    # 4096 finite ones
    cnt = (np.arange(4096, dtype=np.int32) % 7) + 1

    def large():
        tb = fr.track_batch([dict(slot=0, prev_pts=many), dict(slot=1, prev_pts=many[5:6])])
        same_track(tb[0], oracle.track(p0, n0, many, None, 2, 2, 0), "4096 keypoints")
        same_track(tb[1], oracle.track(p0, n0, many[5:6], None, 2, 2, 0), "one keypoint")
        assert int(np.sum(tb[0]["status"] == 0)) >= 1000
        got, ref = fr.detect(tracked, cnt, 4096), oracle.detect(n0, tracked, cnt, None, 4096, 0.01, 0)
        same_detect(got, ref, "4096 tracked points")
        assert ref["n_kept"] >= 1000

    large()
    same_track(fr.track(many[:3]), oracle.track(p0, n0, many[:3], None, 2, 2, 0), "three keypoints after 4096")
    same_detect(fr.detect(tracked[:3], cnt[:3], 40), oracle.detect(n0, tracked[:3], cnt[:3], None, 40, 0.01, 0), "three tracked points after 4096")
    large()
