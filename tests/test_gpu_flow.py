"""The batched pyramidal Lucas-Kanade tracker on the GPU (include/vio_flow.h) against the numpy restatement (tests/flow_reference.py,
order "wave64").

The rule everywhere: the statuses are equal for every keypoint; identical float bits and iteration counts are expected.  As a cap, at
most 2 % of a case's tracked keypoints (at least one) may differ in either, and a differing position by at most 1e-2 px: two orders
below the 1 px F_THRESHOLD at which the tracker's consumer resolves positions, far above float rounding at these magnitudes (ulp 6e-5).
The pyramid is integers and must be exact.  Every case prints its counts (pytest -s).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIFT = (1.3, -0.7)
_cache = {}


@pytest.fixture(scope="module")
def flow_lib(vio, hip_lib):
    return vio.load_flow()


@pytest.fixture()
def fh(flow_lib):
    h = flow_lib.create()
    yield h
    h.close()


def pair(w, h, seed=11):
    key = (w, h, seed)
    if key not in _cache:
        _cache[key] = (fr.texture(w, h, seed=seed), fr.texture(w, h, seed=seed, shift=SHIFT))
    return _cache[key]


def fixture_pair():
    if "fixture" not in _cache:
        _cache["fixture"] = (np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"], np.load(os.path.join(GOLDEN, "flow_image_2.npz"))["image"],
                             np.load(os.path.join(GOLDEN, "flow_keypoints.npz"))["keypoints"])
    return _cache["fixture"]


def grid_pts(w, h, n, margin, seed=2):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], axis=1).astype(np.float32)


def compare(got, ref, name):
    """The rule of the module docstring; returns the number of differing keypoints."""
    out, st, its, cost = ref
    assert np.array_equal(got["status"], st), (name, got["status"], st)
    nan = st == fr.NOT_FINITE
    assert np.all(np.isnan(got["next_pts"][nan])) and np.all(np.isnan(out[nan])), name
    g, r = got["next_pts"][~nan], out[~nan]
    diff = np.any(g.view(np.uint32) != r.view(np.uint32), axis=1) | (got["iterations"][~nan] != its[~nan])
    tracked = int(np.sum(st == fr.OK))
    ndiff = int(diff.sum())
    dist = float(np.max(np.abs(g - r))) if len(g) else 0.0
    print("%s: %d keypoints, %d tracked, %d differ, largest distance %.3g px" % (name, len(st), tracked, ndiff, dist))
    assert ndiff <= max(1, int(0.02 * tracked)), (name, ndiff, tracked)
    assert dist <= 1e-2, (name, dist)
    same = ~diff
    gc, rc = got["cost"][~nan][same], cost[~nan][same]
    assert np.array_equal(np.isnan(gc), np.isnan(rc)) and np.allclose(gc[~np.isnan(gc)], rc[~np.isnan(rc)], rtol=1e-9, atol=1e-9), name
    return ndiff


def run(fh, a, b, pts, guess=None, **cfg):
    fh.set_config(**cfg)
    got = fh.track(a, b, pts, guess)
    ref = fr.multi_level(a, b, pts, guess, order="wave64", **cfg)
    return got, ref


@pytest.mark.parametrize("shape,stride", [((29, 37), None), ((48, 64), 80), ("fixture", None)])
def test_pyramid_is_exact(fh, shape, stride):
    if shape == "fixture":
        img = fixture_pair()[0]
    else:
        img = np.random.RandomState(7).randint(0, 256, size=shape).astype(np.uint8)
        if stride:
            wide = np.zeros((shape[0], stride), dtype=np.uint8)
            wide[:, :shape[1]] = img
            wide[:, shape[1]:] = 255                                    # (what lies between the rows must not be read)
            img = wide[:, :shape[1]]
    levels = 3 if shape == (29, 37) else 4
    fh.set_config(levels=levels)
    got = fh.pyramid(img)
    ref = fr.pyramid(np.ascontiguousarray(img), levels)
    assert len(got) == levels
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.array_equal(g, r)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("half_patch", [1, 4, 5])
def test_small_images(fh, inverse, levels, half_patch):
    a, b = pair(96, 80)
    pts = grid_pts(96, 80, 65, 6)
    compare(*run(fh, a, b, pts, levels=levels, half_patch=half_patch, inverse=inverse), "96x80 L%d h%d inv%d" % (levels, half_patch, inverse))


@pytest.mark.parametrize("inverse", [0, 1])
def test_largest_patch(fh, inverse):
    a, b = pair(160, 128)
    pts = grid_pts(160, 128, 9, 40)
    got, ref = run(fh, a, b, pts, levels=2, half_patch=16, inverse=inverse)
    assert np.all(ref[1] == fr.OK)
    compare(got, ref, "160x128 h16 inv%d" % inverse)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_point_counts_guess_and_one_iteration(fh, inverse, n):
    a, b = pair(64, 48, seed=12)
    pts = grid_pts(64, 48, n, 8)
    guess = (pts + np.array([-1.0, 0.5], dtype=np.float32)).astype(np.float32)
    got, ref = run(fh, a, b, pts, guess, levels=2, inverse=inverse)
    assert got["next_pts"].shape == (n, 2)
    compare(got, ref, "64x48 n%d guess inv%d" % (n, inverse))
    compare(*run(fh, a, b, pts, levels=2, inverse=inverse, max_iter=1), "64x48 n%d max_iter 1 inv%d" % (n, inverse))
    compare(*run(fh, a, b, pts, levels=2, inverse=inverse, early_stop=1), "64x48 n%d early stop inv%d" % (n, inverse))


@pytest.mark.parametrize("inverse", [0, 1])
def test_patches_at_and_over_the_border(fh, inverse):
    a, b = pair(64, 48, seed=12)
    # the template touches the border: the failure, and the position is the input
    pts = np.array([[3.5, 20.0], [20.0, 44.5], [30.0, 24.0]], dtype=np.float32)
    got, ref = run(fh, a, b, pts, levels=1, inverse=inverse)
    compare(got, ref, "template at the border inv%d" % inverse)
    assert list(got["status"][:2]) == [fr.FAIL_LOST, fr.FAIL_LOST] and np.array_equal(got["next_pts"][:2], pts[:2])
    assert list(got["iterations"][:2]) == [0, 0] and np.all(np.isnan(got["cost"][:2]))
    # the patch leaves the image during the iterations: the template is just valid and the flow (-1.3, 0.7) carries the patch out
    pts = np.array([[4.5, 24.0], [30.0, 24.0]], dtype=np.float32)
    got, ref = run(fh, a, b, pts, levels=1, inverse=inverse)
    assert ref[1][0] == fr.FAIL_LOST and ref[2][0] >= 1, (ref[1], ref[2])
    compare(got, ref, "patch leaves the image inv%d" % inverse)
    # 64 x 48 at 4 levels: no patch is valid on the 8 x 6 top level, the finer ones still run
    pts = grid_pts(64, 48, 7, 12)
    got, ref = run(fh, a, b, pts, levels=4, inverse=inverse)
    assert np.any(ref[1] == fr.OK)
    compare(got, ref, "top level skipped inv%d" % inverse)
    # a large border: tracked keypoints outside it get their own code
    got, ref = run(fh, a, b, pts, levels=2, inverse=inverse, border=20)
    assert np.any(ref[1] == fr.FAIL_BORDER)
    compare(got, ref, "border 20 inv%d" % inverse)


@pytest.mark.parametrize("inverse", [0, 1])
def test_flat_image_and_step_edge(fh, inverse):
    flat = np.full((48, 64), 90, dtype=np.uint8)
    pts = np.array([[20.5, 20.25], [2.0, 20.0], [40.0, 30.0]], dtype=np.float32)
    got, ref = run(fh, flat, flat, pts, levels=2, inverse=inverse)          # H is rank 0: dp = 0
    compare(got, ref, "flat inv%d" % inverse)
    assert np.array_equal(got["next_pts"], pts) and list(got["status"]) == [fr.OK, fr.FAIL_LOST, fr.OK]
    edge = np.full((48, 64), 40, dtype=np.uint8)
    edge[:, 32:] = 200
    edge2 = np.full((48, 64), 40, dtype=np.uint8)
    edge2[:, 33:] = 200
    pts = np.array([[31.0, 20.0], [33.5, 30.25], [30.0, 24.0]], dtype=np.float32)
    got, ref = run(fh, edge, edge2, pts, levels=1, inverse=inverse)         # H is rank 1: the basic solution
    compare(got, ref, "step edge inv%d" % inverse)
    assert np.all(got["next_pts"][:, 1] == pts[:, 1])


def test_nan_keypoint_among_good_ones(fh):
    a, b = pair(96, 80)
    pts = grid_pts(96, 80, 9, 10)
    bad = pts.copy()
    bad[4, 0] = np.nan
    guess = pts.copy()
    guess[6, 1] = np.inf
    fh.set_config()
    clean = fh.track(a, b, pts)
    got = fh.track(a, b, bad)
    assert got["status"][4] == fr.NOT_FINITE and np.all(np.isnan(got["next_pts"][4]))
    keep = np.arange(9) != 4
    assert np.array_equal(got["next_pts"][keep].view(np.uint32), clean["next_pts"][keep].view(np.uint32))
    compare(got, fr.multi_level(a, b, bad, order="wave64"), "nan keypoint")
    got = fh.track(a, b, pts, guess)
    assert got["status"][6] == fr.NOT_FINITE and np.all(got["status"][np.arange(9) != 6] != fr.NOT_FINITE)
    compare(got, fr.multi_level(a, b, pts, guess, order="wave64"), "inf guess")


@pytest.mark.parametrize("inverse", [0, 1])
def test_items_of_different_sizes_batch_and_repeat(fh, inverse):
    items = []
    for (w, h, n, seed) in ((96, 80, 21, 11), (64, 48, 5, 12), (160, 128, 30, 11)):
        a, b = pair(w, h, seed)
        items.append(dict(img_prev=a, img_next=b, prev_pts=grid_pts(w, h, n, 10, seed=n)))
    items.insert(1, dict(img_prev=items[0]["img_prev"], img_next=items[0]["img_next"], prev_pts=np.zeros((0, 2), dtype=np.float32)))
    fh.set_config(levels=3, inverse=inverse)
    outs = fh.track_batch(items)
    again = fh.track_batch(items)
    assert len(outs) == 4 and outs[1]["next_pts"].shape == (0, 2)
    for i, (o, o2, it) in enumerate(zip(outs, again, items)):
        for key in ("next_pts", "status", "iterations", "cost"):
            assert o[key].tobytes() == o2[key].tobytes(), (i, key)                  # two calls: the same bits
        compare(o, fr.multi_level(it["img_prev"], it["img_next"], it["prev_pts"], levels=3, inverse=inverse, order="wave64"), "item %d" % i)
    # the same keypoint alone: the same bits as inside the batch
    k = 7
    one = fh.track(items[3]["img_prev"], items[3]["img_next"], items[3]["prev_pts"][k:k + 1])
    for key in ("next_pts", "status", "iterations", "cost"):
        assert one[key].tobytes() == outs[3][key][k:k + 1].tobytes(), key


def test_bad_arguments_write_nothing(vio, fh):
    from vio_amd import flow
    a, b = pair(64, 48, seed=12)
    pts = grid_pts(64, 48, 3, 10)
    nxt = np.full((8, 2), 7.5, dtype=np.float32)
    info = (flow.VioFlowPtInfo * 8)()
    for k in range(8):
        info[k].status = 77

    def call(count=1, items=True, out=True, **kw):
        it = flow.VioFlowItem(64, 48, 64, 3, a.ctypes.data, b.ctypes.data, pts.ctypes.data, None)
        for key, v in kw.items():
            setattr(it, key, v)
        arr = (flow.VioFlowItem * 2)(flow.VioFlowItem(64, 48, 64, 3, a.ctypes.data, b.ctypes.data, pts.ctypes.data, None), it)
        return fh.lib.fn["track_batch"](fh.h, C.c_int32(count), C.addressof(arr) if items else None, nxt.ctypes.data if out else None,
                                        C.addressof(info))

    fh.set_config(levels=4)
    bad = [call(count=-1), call(count=2, items=False), call(count=2, out=False), call(count=2, width=0), call(count=2, height=-3),
           call(count=2, stride=63), call(count=2, n_pts=-1), call(count=2, n_pts=4097), call(count=2, img_prev=None),
           call(count=2, img_next=None), call(count=2, prev_pts=None), call(count=2, width=15, stride=64), call(count=2, width=20000)]
    assert all(st == -1 for st in bad), bad
    assert "item 1" in fh.last_error()
    assert np.all(nxt == 7.5) and all(info[k].status == 77 for k in range(8))
    with pytest.raises(vio.VioError):
        fh.set_config(levels=9)
    with pytest.raises(vio.VioError):
        fh.set_config(half_patch=17)
    with pytest.raises(vio.VioError):
        fh.set_config(max_iter=0)
    out = np.full(64 * 48 * 2, 9, dtype=np.uint8)
    assert fh.lib.fn["pyramid"](fh.h, a.ctypes.data, 64, 48, 60, out.ctypes.data) == -1 and np.all(out == 9)
    fh.set_config(levels=6)
    assert fh.lib.fn["pyramid"](fh.h, a.ctypes.data, 64, 48, 64, out.ctypes.data) == -1 and np.all(out == 9)      # a 2 x 1 level
    assert fh.lib.fn["track_batch"](fh.h, C.c_int32(0), None, None, None) == 0
    assert call(count=1) == -1 and np.all(nxt == 7.5)                        # (64 x 48 has no 6 levels either)
    fh.set_config(levels=4)
    assert call(count=1) == 0 and not np.all(nxt == 7.5)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("half_patch", [4, 10])
def test_fixture_pair(fh, inverse, half_patch):
    im1, im2, kp = fixture_pair()
    key = ("ref", inverse, half_patch)
    if key not in _cache:
        _cache[key] = fr.multi_level(im1, im2, kp, inverse=inverse, half_patch=half_patch, order="wave64")
    fh.set_config(inverse=inverse, half_patch=half_patch)
    got = fh.track(im1, im2, kp)
    assert len(kp) == 170 and np.all(got["status"] == fr.OK)
    compare(got, _cache[key], "fixture h%d inv%d" % (half_patch, inverse))
    t = fh.timing()
    assert all(np.isfinite(v) and v >= 0 for v in t.values())
