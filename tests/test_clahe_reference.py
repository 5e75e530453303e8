"""The numpy restatement of include/vio_clahe.h (tests/clahe_reference.py) against itself: the vectorised formulation and the plain
per-pixel walk agree in every byte, and the properties that follow from the contract hold (a hand-computed flat image, monotone LUTs,
plain equalisation without a clip limit, untouched histograms under a high one, the padding rule, the fixture's clip and its pixels
whose blend lies exactly on a half)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_reference as cr  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def fixture_full():
    return cr.apply(cr.fixture_image(), full=True)


WALK = [(cr.random_image(w, h), 3.0, (8, 8)) for (w, h) in cr.SMALL_SHAPES] + [
    (cr.random_image(23, 19, seed=2), 0.0, (3, 5)), (cr.two_valued(21, 17), 1e-3, (1, 1)), (cr.smooth(40, 24), 40.0, (16, 16)),
    (np.full((12, 20), 9, dtype=np.uint8), 3.0, (8, 8)), (cr.smooth(48, 32), 3.0, (4, 4)), (cr.random_image(5, 3), 2.0, (16, 16))]


@pytest.mark.parametrize("k", range(len(WALK)))
def test_scalar_walk_matches_the_vectorised_form(k):
    img, clip_limit, tiles = WALK[k]
    ref = cr.apply(img, clip_limit, tiles, full=True)
    out, luts = cr.apply_scalar(img, clip_limit, tiles)
    assert luts.tobytes() == ref["luts"].tobytes()
    assert out.tobytes() == ref["out"].tobytes()
    assert ref["out"].shape == img.shape and ref["luts"].shape == (tiles[1], tiles[0], 256)


def test_flat_image_by_hand():
    img = np.full((480, 752), 77, dtype=np.uint8)
    g = cr.geometry(752, 480)
    assert not g["ext"] and (g["tile_w"], g["tile_h"], g["area"], g["clip"]) == (94, 60, 5640, 66)
    hist = cr.tile_hists(img, g)
    assert np.all(hist[:, :, 77] == 5640) and hist.sum() == 752 * 480
    clipped = cr.clip_hists(hist, g["clip"])
    # excess 5574, batch 21, residual 198, step 1: bins 0 .. 197 hold 22 (bin 77: 66 + 22), the others 21
    assert np.all(clipped[:, :, :77] == 22) and np.all(clipped[:, :, 77] == 88) and np.all(clipped[:, :, 198:] == 21)
    assert int(np.cumsum(clipped[0, 0])[77]) == 77 * 22 + 88 == 1782
    assert np.all(clipped.sum(axis=-1) == 5640)                  # (here the whole excess comes back)
    ref = cr.apply(img, full=True)
    assert np.all(ref["luts"][:, :, 77] == 81) and np.all(ref["out"] == 81)


def test_luts_are_non_decreasing(fixture_full):
    assert np.all(np.diff(fixture_full["luts"].astype(np.int64), axis=-1) >= 0)
    for name, img, clip_limit, tiles in cr.config_cases():
        luts = cr.apply(img, clip_limit, tiles, full=True)["luts"]
        assert np.all(np.diff(luts.astype(np.int64), axis=-1) >= 0), name
        assert clip_limit != 0 or np.all(luts[:, :, 255] == 255), name       # (clipping may leave some residual undistributed)


def test_no_clip_limit_is_plain_tile_equalisation():
    img = cr.smooth(96, 72)
    ref = cr.apply(img, 0.0, (8, 8), full=True)
    assert ref["clip"] == 0 and (ref["tile_w"], ref["tile_h"]) == (12, 9)
    for ty in range(8):
        for tx in range(8):
            tile = img[ty * 9:(ty + 1) * 9, tx * 12:(tx + 1) * 12]
            cdf = np.cumsum(np.bincount(tile.reshape(-1), minlength=256))
            plain = np.rint(cdf.astype(F) * (F(255) / F(108))).astype(np.uint8)
            assert np.array_equal(ref["luts"][ty, tx], plain)
            assert ref["luts"][ty, tx, 255] == 255
    # with one tile every pixel blends one LUT with itself: the image's own equalisation
    one = cr.apply(img, 0.0, (1, 1), full=True)
    assert np.array_equal(one["out"], one["luts"][0, 0][img])


def test_high_clip_limit_leaves_the_histograms():
    img = cr.random_image(61, 45, seed=5)
    g = cr.geometry(61, 45, (8, 8), 40.0)
    hist = cr.tile_hists(img, g)
    assert g["clip"] > hist.max()
    assert np.array_equal(cr.clip_hists(hist, g["clip"]), hist)
    assert cr.apply(img, 40.0).tobytes() == cr.apply(img, 0.0).tobytes()
    assert cr.apply(img, 3.0).tobytes() != cr.apply(img, 0.0).tobytes()
    assert cr.geometry(61, 45, (8, 8), 1e300)["clip"] == g["area"] and cr.geometry(61, 45, (8, 8), 1e-3)["clip"] == 1


def test_padding_rule():
    # a direction that divides still gets a whole extra tile count once the other does not divide
    g = cr.geometry(16, 13)
    assert g["ext"] and (g["w_ext"], g["h_ext"], g["tile_w"], g["tile_h"]) == (24, 16, 3, 2)
    g = cr.geometry(13, 16)
    assert g["ext"] and (g["w_ext"], g["h_ext"], g["tile_w"], g["tile_h"]) == (16, 24, 2, 3)
    g = cr.geometry(16, 16)
    assert not g["ext"] and (g["w_ext"], g["h_ext"], g["tile_w"], g["tile_h"]) == (16, 16, 2, 2)
    assert list(cr.reflect_index(5, 14)) == [0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]      # period 2 (n - 1): further than one image
    assert list(cr.reflect_index(2, 6)) == [0, 1, 0, 1, 0, 1] and list(cr.reflect_index(1, 8)) == [0] * 8
    img = cr.random_image(16, 13)
    src = cr.source(img, cr.geometry(16, 13))
    assert src.shape == (16, 24) and np.array_equal(src[:13, :16], img)
    assert np.array_equal(src[:13, 16:], img[:, [14, 13, 12, 11, 10, 9, 8, 7]]) and np.array_equal(src[13:, :16], img[[11, 10, 9], :])
    for v in (0, 77, 255):
        one = cr.apply(np.full((1, 1), v, dtype=np.uint8), full=True)
        assert (one["tile_w"], one["tile_h"], one["clip"]) == (1, 1, 1) and one["out"][0, 0] == 255
        assert np.all(one["luts"][:, :, v:] == 255) and np.all(one["luts"][:, :, :v] == 0)


def test_fixture(fixture_full):
    img = cr.fixture_image()
    assert img.shape == (480, 752)
    ref = fixture_full
    assert (ref["clip"], ref["tile_w"], ref["tile_h"]) == (66, 94, 60)
    assert int(np.sum(ref["hist"].max(axis=-1) > 66)) == 64       # every tile clips
    res = ref["res"]
    half = (res - np.floor(res)) == F(0.5)
    assert int(half.sum()) >= 1                                  # the rounding mode decides these bytes
    print("fixture: %d pixels with res exactly on a half" % int(half.sum()))
    # ... and ties-to-even differs from round-half-up on some of them
    assert np.any(np.floor(res[half] + F(0.5)) != np.rint(res[half]))
    assert ref["out"].tobytes() != img.tobytes() and ref["out"].std() > img.std()


def test_equalizer_interface():
    img = cr.random_image(40, 30)
    eq = cr.Equalizer()
    assert eq.apply(img).tobytes() == cr.apply(img).tobytes()
    eq.set_config(clip_limit=0.0, tiles=(3, 5))
    assert eq.apply(img).tobytes() == cr.apply(img, 0.0, (3, 5)).tobytes()
