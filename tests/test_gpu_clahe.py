"""The batched CLAHE equalisation on the GPU (include/vio_clahe.h) against the numpy restatement (tests/clahe_reference.py).

The rule everywhere: the output bytes and the LUT bytes are equal, and clip, tile_w and tile_h are equal.  There is no tolerance and no
cap on differing cases: histograms, clip and redistribution are integers, a LUT entry is one rounded float32 product and the blend a
fixed sequence of float32 operations, so none may differ.  The shapes come from the apply kernel's block of pixels (TILE_X x TILE_Y of the binding): one below,
at, one above a block, and two blocks and one, in both directions.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_reference as cr  # noqa: E402
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402
from test_frontend_reference import check_frames, fixture_frames  # noqa: E402
from test_gpu_flow import compare as compare_flow  # noqa: E402

pytestmark = pytest.mark.gpu
TX, TY = 128, 16                                # (asserted against the binding in test_tile_constants)
_cache = {}


@pytest.fixture(scope="module")
def clahe_lib(vio, hip_lib):
    return vio.load_clahe()


@pytest.fixture()
def ch(clahe_lib):
    h = clahe_lib.create()
    yield h
    h.close()


def fixture_ref():
    if "fixture" not in _cache:
        img = cr.fixture_image()
        _cache["fixture"] = (img, cr.apply(img, full=True))
    return _cache["fixture"]


def same(got, ref, name):
    assert got["status"] == 0, name
    assert (got["clip"], got["tile_w"], got["tile_h"]) == (ref["clip"], ref["tile_w"], ref["tile_h"]), (name, got["clip"], got["tile_w"], got["tile_h"])
    assert got["luts"].dtype == np.uint8 and got["luts"].shape == ref["luts"].shape, name
    assert got["luts"].tobytes() == ref["luts"].tobytes(), (name, "LUT bytes differ: %d" % int(np.sum(got["luts"] != ref["luts"])))
    assert got["out"].dtype == np.uint8 and got["out"].shape == ref["out"].shape, name
    assert got["out"].tobytes() == ref["out"].tobytes(), (name, "output bytes differ: %d" % int(np.sum(got["out"] != ref["out"])))


def run(ch, img, clip_limit=3.0, tiles=(8, 8), ref=None, name=""):
    ref = cr.apply(np.ascontiguousarray(img), clip_limit, tiles, full=True) if ref is None else ref
    ch.set_config(clip_limit=clip_limit, tiles=tiles)
    got = ch.apply_batch([img], luts=True)[0]
    same(got, ref, name)
    print("%s: %d x %d, tile %d x %d, clip %d" % (name, img.shape[1], img.shape[0], ref["tile_w"], ref["tile_h"], ref["clip"]))
    return got


def test_tile_constants(vio):
    from vio_amd import clahe
    assert (clahe.TILE_X, clahe.TILE_Y) == (TX, TY)


@pytest.mark.parametrize("w,h", cr.SMALL_SHAPES + cr.tile_shapes(TX, TY))
def test_shapes(ch, w, h):
    run(ch, cr.random_image(w, h), name="%dx%d" % (w, h))
    assert ch.apply(cr.random_image(w, h)).shape == (h, w)


def test_configurations(ch):
    """The tile grids 1 x 1, 3 x 5 and 16 x 16, the clip limits 0, 1e-3 (limit 1), 3 and 40, flat, two-valued, smooth and random images,
    and a tile of more than 256 * 4 pixels (every histogram thread loops)."""
    seen = set()
    for name, img, clip_limit, tiles in cr.config_cases():
        got = run(ch, img, clip_limit, tiles, name=name)
        seen.add((got["clip"] == 0, got["clip"] == 1, got["tile_w"] * got["tile_h"] > 256 * 4))
    assert (True, False, False) in seen and (False, True, False) in seen and any(s[2] for s in seen)


def test_stride(ch):
    w, h, s_src, s_dst = 45, 19, 64, 80
    wide = np.full((h, s_src), 255, dtype=np.uint8)              # (what lies between the rows must not be read)
    wide[:, :w] = cr.random_image(w, h)
    img = wide[:, :w]
    assert img.strides[0] == s_src
    ref = cr.apply(np.ascontiguousarray(img), full=True)
    run(ch, img, ref=ref, name="strided source")
    canvas = np.full((h, s_dst), 99, dtype=np.uint8)             # ... and what lies between the result's rows is not written
    dst = canvas[:, :w]
    ch.set_config()
    got = ch.apply_batch([img], out=[dst])[0]
    assert got is dst and dst.tobytes() == ref["out"].tobytes() and np.all(canvas[:, w:] == 99)
    # a source read column by column (no contiguous rows) is copied by the binding
    assert ch.apply(np.asfortranarray(np.ascontiguousarray(img))).tobytes() == ref["out"].tobytes()


def test_fixture(ch):
    img, ref = fixture_ref()
    got = run(ch, img, ref=ref, name="fixture")
    assert got["clip"] == 66 and (got["tile_w"], got["tile_h"]) == (94, 60)
    res = ref["res"]
    assert int(np.sum((res - np.floor(res)) == np.float32(0.5))) > 0          # pixels whose byte the rounding mode and contraction decide
    t = ch.timing()
    assert len(t) == 4 and all(np.isfinite(v) and v >= 0 for v in t.values()), t
    run(ch, img, 3.0, (16, 16), name="fixture, 16 x 16 tiles")                # (64 KB of LUTs: the largest staging)


def batch_images():
    return [cr.random_image(2 * TX + 1, TY + 3, seed=3), cr.smooth(61, 45), cr.two_valued(TX - 3, 2 * TY)]


def test_batch_repeat_and_alone(ch):
    imgs = batch_images()
    assert len({im.shape for im in imgs}) == 3
    ch.set_config(clip_limit=2.0, tiles=(8, 8))
    outs = ch.apply_batch(imgs, luts=True)
    again = ch.apply_batch(imgs, luts=True)
    for i, (o, o2, im) in enumerate(zip(outs, again, imgs)):
        same(o, cr.apply(im, 2.0, (8, 8), full=True), "item %d" % i)
        assert o["out"].tobytes() == o2["out"].tobytes() and o["luts"].tobytes() == o2["luts"].tobytes(), i      # two calls: the same bytes
        alone = ch.apply_batch([im], luts=True)[0]                                  # alone: the same bytes as inside the batch
        assert alone["out"].tobytes() == o["out"].tobytes() and alone["luts"].tobytes() == o["luts"].tobytes(), i
        assert (alone["clip"], alone["tile_w"], alone["tile_h"]) == (o["clip"], o["tile_w"], o["tile_h"])
    plain = ch.apply_batch(imgs)                                                    # without the LUTs: the same images
    assert all(p.tobytes() == o["out"].tobytes() for p, o in zip(plain, outs))
    assert ch.apply_batch([]) == []


def test_bad_arguments_write_nothing(vio, ch):
    from vio_amd import clahe
    w, h = 40, 20
    img = cr.random_image(w, h)
    dst = np.full((h, w), 7, dtype=np.uint8)
    luts = np.full((8, 8, 256), 9, dtype=np.uint8)
    both = np.zeros(2 * w * h, dtype=np.uint8)                   # a source and a destination that share bytes
    res = (clahe.VioClaheResult * 2)()
    for k in range(2):
        res[k].status, res[k].clip, res[k].tile_w, res[k].tile_h = 55, 66, 77, 88

    def item(**kw):
        it = clahe.VioClaheItem(w, h, w, w, img.ctypes.data, dst.ctypes.data, luts.ctypes.data)
        for key, v in kw.items():
            setattr(it, key, v)
        return it

    def call(count=2, items=True, out=True, **kw):
        arr = (clahe.VioClaheItem * 2)(item(), item(**kw))
        return ch.lib.fn["apply_batch"](ch.h, C.c_int32(count), C.addressof(arr) if items else None, C.addressof(res) if out else None)

    ch.set_config()
    bad = [call(count=-1), call(count=4097), call(items=False), call(out=False), call(width=0), call(height=-3), call(width=20000),
           call(height=16385), call(src_stride=w - 1), call(dst_stride=w - 1), call(src=None), call(dst=None),
           call(src=both.ctypes.data, dst=both.ctypes.data), call(src=both.ctypes.data, dst=both.ctypes.data + w * h - 1),
           call(src=both.ctypes.data + 5, dst=both.ctypes.data)]
    assert all(st == -1 for st in bad), bad
    assert "item 1" in ch.last_error()
    assert np.all(dst == 7) and np.all(luts == 9) and np.all(both == 0)
    assert all(res[k].status == 55 and res[k].clip == 66 and res[k].tile_w == 77 and res[k].tile_h == 88 for k in range(2))
    for cfg in (dict(clip_limit=-1.0), dict(clip_limit=float("nan")), dict(clip_limit=float("inf")), dict(tiles=(0, 8)), dict(tiles=(8, 17)),
                dict(tiles=(-1, 8)), dict(tiles=(17, 1))):
        with pytest.raises(vio.VioError):
            ch.set_config(**cfg)
    assert ch.lib.fn["apply_batch"](ch.h, C.c_int32(0), None, None) == 0
    # adjacent, not overlapping: allowed; and the good call writes
    assert call(src=both.ctypes.data, dst=both.ctypes.data + w * h, luts=None) == 0
    ref = cr.apply(img, full=True)
    assert res[0].status == 0 and (res[0].clip, res[0].tile_w, res[0].tile_h) == (ref["clip"], ref["tile_w"], ref["tile_h"])
    assert dst.tobytes() == ref["out"].tobytes() and luts.tobytes() == ref["luts"].tobytes()
    assert np.all(both[:w * h] == 0) and both[w * h:].tobytes() == cr.apply(np.zeros((h, w), dtype=np.uint8)).tobytes()


class Spy:
    """Records what a handle's method was given and what it returned."""

    def __init__(self, inner, method):
        self.inner, self.calls = inner, []
        setattr(self, method, self._call(getattr(inner, method)))
        if hasattr(inner, "set_config"):
            self.set_config = inner.set_config

    def _call(self, fn):
        def f(*a, **kw):
            out = fn(*a, **kw)
            self.calls.append((a, kw, out))
            return out
        return f


def test_front_end(vio, ch):
    """FeatureTracker over the flow, detect and clahe handles: the invariants hold, and every handle's step equals its restatement on
    what the front end gave it (the equaliser and the detector in every byte, the tracker by the rule of test_gpu_flow.py)."""
    frames = fixture_frames()
    fl, dh = vio.load_flow().create(), vio.load_detect().create()
    try:
        ch.set_config()
        eq, tr, de = Spy(ch, "apply"), Spy(fl, "track"), Spy(dh, "detect")
        ft = vio.FeatureTracker(tr, de, max_cnt=150, min_dist=30, equalizer=eq)
        outs = check_frames(ft, frames)
        eq0 = fixture_ref()[1]["out"]
        eq1 = cr.apply(frames[1])
        assert [c[2].tobytes() for c in eq.calls] == [eq0.tobytes(), eq1.tobytes(), eq0.tobytes()]
        assert ft.prev_img.tobytes() == eq1.tobytes() and ft.cur_img.tobytes() == eq0.tobytes()
        # the detector saw the equalised frames; its first two answers against the restatement
        assert [c[0][0].tobytes() for c in de.calls] == [eq0.tobytes(), eq1.tobytes(), eq0.tobytes()]
        for (a, kw, got) in de.calls[:2]:
            ref = dr.detect(a[0], kw["tracked"], kw["track_cnt"], kw["mask"], kw["max_total"], min_distance=30)
            assert np.array_equal(got["keep_order"], ref["keep_order"]) and got["new_pts"].tobytes() == ref["new_pts"].tobytes()
        assert np.array_equal(outs[0]["pts"], de.calls[0][2]["new_pts"])
        # the tracker saw equalised pairs; its first answer against the restatement
        (a, kw, got) = tr.calls[0]
        assert len(tr.calls) == 2 and a[0].tobytes() == eq0.tobytes() and a[1].tobytes() == eq1.tobytes()
        compare_flow(got, fr.multi_level(a[0], a[1], a[2], None, order="wave64"), "front end, frame 2")
    finally:
        fl.close()
        dh.close()
