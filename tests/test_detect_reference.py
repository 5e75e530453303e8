"""The numpy restatement of the corner detector (tests/detect_reference.py, the contract of include/vio_detect.h) against what the
contract promises: where corners are, the invariants of setMask and of the selection, the integer bounds, the degenerate images."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def image(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"] if name == "fixture" else fr.texture(160, 128, seed=11)
        _cache[name + "/R"] = dr.response(_cache[name])
    return _cache[name], _cache[name + "/R"]


def test_rectangle_corners():
    img = np.zeros((60, 80), dtype=np.uint8)
    img[20:41, 25:56] = 255
    out = dr.detect(img, min_distance=5, max_total=4)
    assert out["n_new"] == 4
    corners = {(25, 20), (55, 20), (25, 40), (55, 40)}
    found = set()
    for x, y in out["new_pts"]:
        near = [c for c in corners if abs(c[0] - x) <= 1 and abs(c[1] - y) <= 1]
        assert len(near) == 1, (x, y)
        found.add(near[0])
    assert found == corners


def check_invariants(img, R, out, pts, cnt, mask, max_total, min_distance):
    new = out["new_pts"].astype(np.int64)
    d2 = min_distance ** 2
    for i in range(len(new)):
        d = np.sum((new[:i] - new[i]) ** 2, axis=1)
        assert np.all(d >= d2), i
    kept = dr.round_points(pts)[out["keep_order"]] if len(out["keep_order"]) else np.zeros((0, 2), dtype=np.int64)
    for p in new:
        assert np.all(np.sum((kept - p) ** 2, axis=1) > d2)
        assert mask is None or mask[p[1], p[0]] != 0
    r = R[new[:, 1], new[:, 0]]
    assert np.all(r[1:] <= r[:-1]) and np.all(r > 0)
    assert out["n_kept"] + out["n_new"] <= max_total
    assert out["n_kept"] == len(out["keep_order"]) and out["n_new"] == len(out["new_pts"])
    for i in range(len(kept)):
        assert np.all(np.sum((kept[:i] - kept[i]) ** 2, axis=1) > d2)
        assert mask is None or mask[kept[i, 1], kept[i, 0]] != 0
    kc = np.asarray(cnt)[out["keep_order"]]
    assert np.all(kc[1:] <= kc[:-1])


@pytest.mark.parametrize("name", ["fixture", "texture"])
def test_invariants(name):
    img, R = image(name)
    h, w = img.shape
    first = dr.detect(img, R=R)
    assert first["n_kept"] == 0 and 0 < first["n_new"] <= 150 and first["n_candidates"] >= first["n_new"]
    check_invariants(img, R, first, np.zeros((0, 2)), [], None, 150, 30)
    # fed back as tracked points with mixed counts, a user mask with a zero region, other settings
    rng = np.random.RandomState(5)
    pts = np.concatenate([first["new_pts"][:60], first["new_pts"][:20] + np.float32(1.4)]).astype(np.float32)
    cnt = rng.randint(1, 6, size=len(pts)).astype(np.int32)
    mask = np.full((h, w), 255, dtype=np.uint8)
    mask[:, : w // 3] = 0
    for (max_total, md, m) in ((150, 30, None), (150, 30, mask), (70, 10, mask), (1000, 10, None)):
        out = dr.detect(img, pts, cnt, m, max_total, min_distance=md, R=R)
        check_invariants(img, R, out, pts, cnt, m, max_total, md)
        if m is not None:
            assert out["n_kept"] < len(pts)
    if name == "fixture":
        dense = dr.detect(img, max_total=1000, min_distance=10, R=R)
        assert dense["n_new"] > first["n_new"]
        again = dr.detect(img, first["new_pts"][:100], np.ones(100), R=R)
        assert again["n_kept"] + again["n_new"] <= 150 and again["n_candidates"] < first["n_candidates"] and again["n_new"] > 0


def test_set_mask_prefers_long_tracks_then_low_indices():
    pts = np.array([[20.0, 20.0], [23.0, 20.0], [60.0, 20.0], [60.4, 20.4], [90.0, 50.0]], dtype=np.float32)
    keep, allowed = dr.set_mask((80, 120), pts, [1, 5, 3, 3, 2], min_distance=10)
    assert list(keep) == [1, 2, 4]                       # the higher count of (0, 1), the lower index of (2, 3); counts descending
    assert not allowed[20, 23] and not allowed[20, 33] and allowed[20, 34] and not allowed[26, 31] and allowed[27, 31]
    keep, _ = dr.set_mask((80, 120), pts, [7, 5, 3, 3, 2], min_distance=10)
    assert list(keep) == [0, 2, 4]
    # ties to even: 20.5 -> 20, 21.5 -> 22
    assert dr.round_points([[20.5, 21.5], [0.5, 1.5]]).tolist() == [[20, 22], [0, 2]]
    # min_distance 0: only points on one pixel exclude each other
    keep, _ = dr.set_mask((80, 120), np.array([[5.2, 5.0], [4.9, 5.1], [6.0, 5.0]], dtype=np.float32), [1, 1, 1], min_distance=0)
    assert list(keep) == [0, 2]


def test_bounds_on_the_steepest_images():
    """R >= 0 and a radicand below 2^53 on alternating 0 / 255 columns, and on columns alternating in pairs.  The Sobel kernel is a
    central difference, so single alternating columns have gx = 0 away from the border; pairs (0 0 255 255) have |gx| = 1020 in every
    column, which is what reaches the bounds of the contract."""
    single = np.zeros((16, 24), dtype=np.uint8)
    single[:, ::2] = 255
    pairs = np.zeros((16, 24), dtype=np.uint8)
    pairs[:, (np.arange(24) // 2) % 2 == 1] = 255
    gx, gy = dr.sobel(pairs)
    assert np.abs(gx[:, 1:-1]).min() == np.abs(gx).max() == 1020 and np.abs(gy).max() == 0
    a, b, c = dr.box_sums(pairs)
    assert a.max() == 9 * 1020 ** 2 == 9363600
    diag = np.zeros((24, 24), dtype=np.uint8)
    diag[((np.arange(24)[:, None] + np.arange(24)[None, :]) // 2) % 2 == 1] = 255
    for im in (single, single.T.copy(), pairs, pairs.T.copy(), diag, np.random.RandomState(3).randint(0, 2, size=(40, 40)).astype(np.uint8) * 255):
        a, b, c = dr.box_sums(im)
        assert int(dr.radicand(a, b, c).max()) <= 4.4e14 < 2 ** 53 and max(int(a.max()), int(c.max())) <= 9363600
        R = dr.response(im)
        assert np.all(R >= 0) and np.all(np.isfinite(R))
    assert np.all(image("fixture")[1] >= 0)


def test_flat_and_tiny_images():
    out = dr.detect(np.full((20, 30), 77, dtype=np.uint8))
    assert out["max_response"] == 0.0 and out["n_candidates"] == 0 and out["n_new"] == 0
    for shape in ((1, 1), (2, 5), (5, 2)):
        out = dr.detect(np.random.RandomState(1).randint(0, 256, size=shape).astype(np.uint8))
        assert out["n_candidates"] == 0 and out["n_new"] == 0
    # a disc over the whole image: maxR is over nothing
    img = fr.texture(24, 16, seed=3)
    out = dr.detect(img, np.array([[12.0, 8.0]], dtype=np.float32), [4], min_distance=40)
    assert out["n_kept"] == 1 and out["max_response"] == 0.0 and out["n_new"] == 0
    out = dr.detect(img, np.array([[np.nan, 8.0]], dtype=np.float32), [4])
    assert out["status"] == dr.NOT_FINITE and out["n_kept"] == 0
