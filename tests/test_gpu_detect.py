"""The batched corner detector on the GPU (include/vio_detect.h) against the numpy restatement (tests/detect_reference.py).

The rule everywhere: the response map is equal in every bit, n_kept, n_new, n_candidates and the bits of max_response are equal,
keep_order and new_pts are equal element for element.  There is no tolerance and no cap on differing cases: the contract keeps every
quantity an integer up to one correctly rounded square root, so none may differ.  The shapes come from the kernels' tile (TILE_X x
TILE_Y of the binding): one below, at, one above a tile, and two tiles and one, in both directions.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402
from test_frontend_reference import check_frames, fixture_frames  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TX, TY = 32, 8                                  # (asserted against the binding in test_tile_constants)
_cache = {}


@pytest.fixture(scope="module")
def detect_lib(vio, hip_lib):
    return vio.load_detect()


@pytest.fixture()
def dh(detect_lib):
    h = detect_lib.create()
    yield h
    h.close()


def fixture_image():
    if "fixture" not in _cache:
        img = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
        _cache["fixture"] = (img, dr.response(img))
    return _cache["fixture"]


def random_image(w, h, seed=7):
    return np.random.RandomState(seed + 131 * w + h).randint(0, 256, size=(h, w)).astype(np.uint8)


def same(got, ref, name):
    assert got["status"] == ref["status"], (name, got["status"], ref["status"])
    for k in ("n_kept", "n_new", "n_candidates"):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    assert np.float64(got["max_response"]).tobytes() == np.float64(ref["max_response"]).tobytes(), (name, got["max_response"], ref["max_response"])
    assert np.array_equal(got["keep_order"], ref["keep_order"]), (name, got["keep_order"], ref["keep_order"])
    assert got["new_pts"].dtype == np.float32 and got["new_pts"].tobytes() == ref["new_pts"].astype(np.float32).tobytes(), name
    print("%s: kept %d, candidates %d, new %d" % (name, got["n_kept"], got["n_candidates"], got["n_new"]))


def run(dh, img, tracked=None, track_cnt=None, mask=None, max_total=150, quality=0.01, min_distance=30, R=None, name=""):
    dh.set_config(quality=quality, min_distance=min_distance)
    got = dh.detect(img, tracked, track_cnt, mask, max_total)
    ref = dr.detect(np.ascontiguousarray(img), tracked, track_cnt, None if mask is None else np.ascontiguousarray(mask), max_total, quality,
                    min_distance, R=R)
    same(got, ref, name)
    return got, ref


def test_tile_constants(vio):
    from vio_amd import detect
    assert (detect.TILE_X, detect.TILE_Y) == (TX, TY)


SHAPES = [(1, 1), (5, 2), (2, 5), (3, 3), (17, 13)] + [(w, h) for w in (TX - 1, TX, TX + 1, 2 * TX + 1) for h in (TY - 1, TY, TY + 1, 2 * TY + 1)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_tiny_images(dh, w, h):
    img = random_image(w, h)
    R = dr.response(img)
    got = dh.response(img)
    assert got.shape == R.shape and got.tobytes() == R.tobytes(), (w, h, int(np.sum(got != R)))
    run(dh, img, min_distance=2, max_total=4096, R=R, name="%dx%d all" % (w, h))
    # three tracked points (where the image has room), a stop at n_want, a disc that reaches over tile edges
    n = min(3, w * h)
    pix = np.random.RandomState(w + h).choice(w * h, size=n, replace=False)
    pts = np.stack([pix % w, pix // w], axis=1).astype(np.float32)
    run(dh, img, pts, [2, 1, 2][:n], min_distance=3, max_total=12, R=R, name="%dx%d tracked" % (w, h))


def test_stride_and_user_mask(dh):
    w, h, stride = 45, 19, 64
    wide = np.full((h, stride), 255, dtype=np.uint8)            # (what lies between the rows must not be read)
    wide[:, :w] = random_image(w, h)
    img = wide[:, :w]
    assert img.strides[0] == stride
    R = dr.response(np.ascontiguousarray(img))
    assert dh.response(img).tobytes() == R.tobytes()
    wide_mask = np.zeros((h, stride), dtype=np.uint8)
    wide_mask[:, :w] = 1
    wide_mask[5:12, 10:30] = 0                                  # the mask's own zero region
    wide_mask[:, w:] = 255
    mask = wide_mask[:, :w]
    pts = np.array([[12.0, 7.0], [40.0, 3.0], [20.4, 15.6], [3.0, 3.0]], dtype=np.float32)      # the first is on a zero mask pixel
    got, ref = run(dh, img, pts, [9, 1, 1, 1], mask, max_total=40, min_distance=4, R=R, name="stride + mask")
    assert 0 not in got["keep_order"] and got["n_kept"] == 3 and got["n_new"] > 0
    assert np.all(mask[got["new_pts"][:, 1].astype(int), got["new_pts"][:, 0].astype(int)] != 0)
    no_mask, _ = run(dh, img, pts, [9, 1, 1, 1], None, max_total=40, min_distance=4, R=R, name="stride, no mask")
    assert no_mask["n_kept"] == 4 and no_mask["n_candidates"] != got["n_candidates"]


@pytest.mark.parametrize("min_distance", [0, 1, 5])
def test_ties(dh, min_distance):
    yy, xx = np.mgrid[0:48, 0:64]
    img = ((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)
    R = dr.response(img)
    ref = dr.detect(img, min_distance=min_distance, R=R)
    rv = R.reshape(-1)[ref["candidates"]]
    assert len(rv) > 100 and len(np.unique(rv)) < len(rv) / 4, (len(rv), len(np.unique(rv)))    # equal responses: the index tie-break decides
    assert dh.response(img).tobytes() == R.tobytes()
    run(dh, img, min_distance=min_distance, R=R, name="checkerboard d%d" % min_distance)
    run(dh, img, min_distance=min_distance, max_total=1000, R=R, name="checkerboard d%d all" % min_distance)
    run(dh, img, min_distance=min_distance, max_total=7, quality=1.0, R=R, name="checkerboard d%d quality 1" % min_distance)


def test_limits(dh):
    w, h = 2 * TX + 5, 3 * TY + 2
    img = fr.texture(w, h, seed=21)
    R = dr.response(img)
    n_all = dr.detect(img, min_distance=3, max_total=4096, R=R)["n_new"]
    assert n_all > 3
    for max_total in (0, 1, n_all, 4096):
        got, _ = run(dh, img, min_distance=3, max_total=max_total, R=R, name="max_total %d" % max_total)
        assert got["n_new"] == min(max_total, n_all)
    rng = np.random.RandomState(4)
    for n in (0, 1, 65):
        pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)
        cnt = rng.randint(1, 4, size=n).astype(np.int32)        # many equal counts
        run(dh, img, pts, cnt, min_distance=3, max_total=80, R=R, name="n_tracked %d" % n)
        run(dh, img, pts, np.ones(n, dtype=np.int32), min_distance=0, max_total=80, R=R, name="n_tracked %d equal counts d0" % n)
    # as many kept points as max_total, and more: nothing to detect
    pts = np.stack([np.arange(8) * 8.0 + 2, np.full(8, 5.0)], axis=1).astype(np.float32)
    for max_total in (8, 5):
        got, _ = run(dh, img, pts, np.arange(8), min_distance=3, max_total=max_total, R=R, name="kept >= max_total %d" % max_total)
        assert got["n_kept"] == 8 and got["n_new"] == 0 and got["n_candidates"] > 0
    # two points rounding to one pixel (ties to even: 10.5 -> 10, 9.5 -> 10), equal counts: the lower index stays
    pts = np.array([[10.5, 6.0], [9.5, 6.4], [30.0, 20.0]], dtype=np.float32)
    got, _ = run(dh, img, pts, [3, 3, 3], min_distance=0, max_total=30, R=R, name="one pixel twice")
    assert list(got["keep_order"]) == [0, 2]
    got, _ = run(dh, img, pts, [3, 4, 5], min_distance=3, max_total=30, R=R, name="one pixel twice, counts")
    assert list(got["keep_order"]) == [2, 1]
    # a tracked point on a zero mask pixel
    mask = np.ones((h, w), dtype=np.uint8)
    mask[6, 10] = 0
    got, _ = run(dh, img, pts, [3, 3, 3], mask, min_distance=2, max_total=30, R=R, name="tracked on a zero mask pixel")
    assert list(got["keep_order"]) == [2]
    # a disc over the whole image: maxR is over nothing; and a mask of zeros
    got, _ = run(dh, img, np.array([[30.0, 12.0]], dtype=np.float32), [1], min_distance=200, max_total=30, R=R, name="disc over everything")
    assert got["n_kept"] == 1 and got["max_response"] == 0.0 and got["n_candidates"] == 0 and got["n_new"] == 0
    got, _ = run(dh, img, None, None, np.zeros((h, w), dtype=np.uint8), R=R, name="mask of zeros")
    assert got["max_response"] == 0.0 and got["n_new"] == 0
    flat, _ = run(dh, np.full((h, w), 90, dtype=np.uint8), name="flat")
    assert flat["max_response"] == 0.0 and flat["n_candidates"] == 0


@pytest.mark.parametrize("case", ["defaults", "fed back", "dense"])
def test_fixture(dh, case):
    img, R = fixture_image()
    if "first" not in _cache:
        _cache["first"] = dr.detect(img, R=R)
    first = _cache["first"]
    if case == "defaults":
        assert dh.response(img).tobytes() == R.tobytes()
        got, ref = run(dh, img, R=R, name="fixture")
        assert got["n_new"] == first["n_new"] > 100 and got["n_candidates"] > 1000
    elif case == "fed back":
        got, ref = run(dh, img, first["new_pts"][:100], np.ones(100, dtype=np.int32), R=R, name="fixture, 100 tracked")
        assert got["n_kept"] >= 99 and got["n_kept"] + got["n_new"] == 150
    else:
        got, ref = run(dh, img, max_total=1000, min_distance=10, R=R, name="fixture d10 max 1000")
        assert got["n_new"] > 500
    t = dh.timing()
    assert len(t) == 6 and all(np.isfinite(v) and v >= 0 for v in t.values()), t


def batch_items():
    rng = np.random.RandomState(9)
    items = []
    for (w, h, n, max_total) in ((2 * TX + 1, TY + 3, 5, 30), (TX - 3, 2 * TY, 0, 10), (3 * TX, 3 * TY + 1, 20, 60), (2, 2, 1, 5)):
        pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)
        items.append(dict(img=random_image(w, h, seed=3), tracked=pts, track_cnt=rng.randint(1, 5, size=n).astype(np.int32), mask=None,
                          max_total=max_total))
    items.insert(2, dict(img=items[0]["img"], tracked=None, track_cnt=None, mask=None, max_total=0))    # an empty one: nothing tracked, nothing wanted
    return items


KEYS = ("keep_order", "new_pts")


def result_bytes(o):
    return (o["status"], o["n_kept"], o["n_new"], o["n_candidates"], np.float64(o["max_response"]).tobytes()) + tuple(o[k].tobytes() for k in KEYS)


def test_batch_repeat_and_alone(dh):
    items = batch_items()
    dh.set_config(min_distance=4)
    outs = dh.detect_batch(items)
    again = dh.detect_batch(items)
    assert len(outs) == len(items) == 5 and outs[2]["n_new"] == 0 and outs[2]["n_kept"] == 0 and outs[2]["n_candidates"] > 0
    for i, (o, o2, it) in enumerate(zip(outs, again, items)):
        assert result_bytes(o) == result_bytes(o2), i                                   # two calls: the same bytes
        same(o, dr.detect(it["img"], it["tracked"], it["track_cnt"], None, it["max_total"], min_distance=4), "item %d" % i)
        alone = dh.detect_batch([it])[0]                                                # alone: the same bytes as inside the batch
        assert result_bytes(alone) == result_bytes(o), i
    assert dh.detect_batch([]) == []


def test_nan_item(dh):
    items = batch_items()[:3]
    dh.set_config(min_distance=4)
    clean = dh.detect_batch(items)
    bad = [dict(it) for it in items]
    pts = np.array([[3.0, 2.0], [np.nan, 4.0], [8.0, 5.0]], dtype=np.float32)
    bad[1] = dict(bad[1], tracked=pts, track_cnt=[1, 2, 3])
    outs = dh.detect_batch(bad)                                                         # (does not raise)
    assert outs[1]["status"] == dr.NOT_FINITE and outs[1]["n_kept"] == 0 and outs[1]["n_new"] == 0 and len(outs[1]["keep_order"]) == 0
    assert "item 1" in dh.last_error()
    for i in (0, 2):
        assert outs[i]["status"] == 0 and result_bytes(outs[i]) == result_bytes(clean[i]), i
    bad[1] = dict(bad[1], tracked=np.array([[3.0, np.inf]], dtype=np.float32), track_cnt=[1])
    assert dh.detect_batch(bad)[1]["status"] == dr.NOT_FINITE


def test_bad_arguments_write_nothing(vio, dh):
    from vio_amd import detect
    w, h = 40, 20
    img = random_image(w, h)
    pts = np.array([[5.0, 5.0], [20.0, 10.0], [30.0, 15.0]], dtype=np.float32)
    cnt = np.array([1, 2, 3], dtype=np.int32)
    keep = np.full(16, 77, dtype=np.int32)
    new = np.full((64, 2), 7.5, dtype=np.float32)
    res = (detect.VioDetectResult * 2)()
    for k in range(2):
        res[k].status, res[k].n_new, res[k].max_response = 55, 66, 8.5
    far = np.array([[5.0, 5.0], [39.6, 10.0], [30.0, 15.0]], dtype=np.float32)          # 39.6 rounds to 40: outside
    low = np.array([[5.0, 5.0], [20.0, -0.6], [30.0, 15.0]], dtype=np.float32)
    huge = np.array([[5.0, 5.0], [20.0, 3e38], [30.0, 15.0]], dtype=np.float32)

    def item(**kw):
        it = detect.VioDetectItem(w, h, w, 3, 20, 0, img.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, keep.ctypes.data, new.ctypes.data)
        for key, v in kw.items():
            setattr(it, key, v)
        return it

    def call(count=2, items=True, out=True, **kw):
        arr = (detect.VioDetectItem * 2)(item(), item(**kw))
        return dh.lib.fn["batch"](dh.h, C.c_int32(count), C.addressof(arr) if items else None, C.addressof(res) if out else None)

    dh.set_config(min_distance=3)
    bad = [call(count=-1), call(items=False), call(out=False), call(width=0), call(height=-3), call(width=20000), call(stride=w - 1),
           call(n_tracked=-1), call(n_tracked=4097), call(max_total=-1), call(max_total=4097), call(img=None), call(tracked=None),
           call(track_cnt=None), call(keep_order=None), call(new_pts=None), call(tracked=far.ctypes.data), call(tracked=low.ctypes.data),
           call(tracked=huge.ctypes.data)]
    assert all(st == -1 for st in bad), bad
    assert "item 1" in dh.last_error()
    assert np.all(keep == 77) and np.all(new == 7.5) and all(res[k].status == 55 and res[k].n_new == 66 and res[k].max_response == 8.5 for k in range(2))
    for cfg in (dict(quality=0.0), dict(quality=-0.5), dict(quality=1.5), dict(quality=float("nan")), dict(min_distance=-1)):
        with pytest.raises(vio.VioError):
            dh.set_config(**cfg)
    out = np.full((h, w), 9.0)
    assert dh.lib.fn["response"](dh.h, img.ctypes.data, w, h, w - 1, out.ctypes.data) == -1 and np.all(out == 9.0)
    assert dh.lib.fn["response"](dh.h, None, w, h, w, out.ctypes.data) == -1 and np.all(out == 9.0)
    assert dh.lib.fn["batch"](dh.h, C.c_int32(0), None, None) == 0
    assert call() == 0 and res[1].status == 0 and res[1].n_kept == 3 and list(keep[:3]) == [2, 1, 0] and not np.all(new == 7.5)
    assert np.all(keep[3:] == 77) and np.all(new[res[1].n_new:] == 7.5)                 # nothing past the item's rows


def test_front_end(vio, detect_lib, dh):
    fl = vio.load_flow().create()
    try:
        ft = vio.FeatureTracker(fl, dh, max_cnt=150, min_dist=30)
        outs = check_frames(ft, fixture_frames())
        first = dr.detect(fixture_frames()[0], R=fixture_image()[1])
        assert np.array_equal(outs[0]["pts"], first["new_pts"])
        assert np.sum(outs[1]["track_cnt"] == 2) >= 0.8 * first["n_new"]
        assert np.sum(outs[2]["track_cnt"] == 3) >= 0.7 * first["n_new"]
    finally:
        fl.close()
