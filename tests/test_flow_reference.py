"""The numpy restatement of the pyramidal Lucas-Kanade tracker (tests/flow_reference.py) on its own: the pyramid, the 2 x 2 solve, the
recovery of a known shift, the degenerate patches, and the two summation orders on the fixture pair.

Shift recovery.  A smooth seeded texture (flow_reference.texture, 160 x 128) is sampled again 1.3 px to the right and 0.7 px up, so
every keypoint's true flow is (-1.3, 0.7).  The restatement's own worst error over the 20 interior keypoints, measured:
    forward   0.1085 px at 1, 2, 3 and 4 levels
    inverse   0.1121 px at 1, 2, 3 and 4 levels
(the step scaled by 32 / 26 without a stop on a rising cost and the 8-bit texture bound it, not the level count).  The bar is 10 x
the larger, 1.12 px, and every keypoint must track.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as fr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIFT = (1.3, -0.7)
SHIFT_BAR = 1.12


def fixture_pair():
    im1 = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
    im2 = np.load(os.path.join(GOLDEN, "flow_image_2.npz"))["image"]
    kp = np.load(os.path.join(GOLDEN, "flow_keypoints.npz"))["keypoints"]
    return im1, im2, kp


def test_pyr_down_of_a_constant_is_the_constant():
    for c in (0, 1, 127, 255):
        out = fr.pyr_down(np.full((30, 44), c, dtype=np.uint8))
        assert out.shape == (15, 22) and np.all(out == c)


def test_pyr_down_of_odd_sizes():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=(29, 37)).astype(np.uint8)
    out = fr.pyr_down(img)
    assert out.shape == (14, 18) and out.dtype == np.uint8
    # an interior pixel by the definition: rows and columns 2y - 2 .. 2y + 2
    k = np.array([1, 4, 6, 4, 1])
    for (y, x) in ((3, 5), (10, 12), (13, 17)):
        patch = np.pad(img.astype(np.int64), 2, mode="reflect")[2 * y:2 * y + 5, 2 * x:2 * x + 5]
        assert out[y, x] == (int(k @ patch @ k) + 128) >> 8
    assert [a.shape for a in fr.pyramid(img, 3)] == [(29, 37), (14, 18), (7, 9)]


def test_scharr_is_the_kernel_with_reflect_101():
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(9, 11)).astype(np.uint8)
    gx, gy = fr.scharr(img)
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]])
    for (y, x) in ((0, 0), (4, 5), (8, 10), (0, 10)):
        win = p[y:y + 3, x:x + 3]
        assert gx[y, x] == np.sum(kx * win) and gy[y, x] == np.sum(kx.T * win)


def test_solve2_full_rank_and_degenerate():
    rng = np.random.RandomState(5)
    for _ in range(50):
        j = rng.randn(8, 2) * rng.uniform(0.1, 100)
        H, b = j.T @ j, rng.randn(2)
        d = fr.solve2(H, b)
        assert np.allclose(d, np.linalg.solve(H, b), rtol=1e-9, atol=1e-12)
    assert np.array_equal(fr.solve2(np.zeros((2, 2)), [1.0, 2.0]), [0.0, 0.0])                  # rank 0
    assert np.array_equal(fr.solve2([[4.0, 0.0], [0.0, 0.0]], [2.0, 5.0]), [0.5, 0.0])          # rank 1: the basic solution
    assert np.array_equal(fr.solve2([[0.0, 0.0], [0.0, 4.0]], [2.0, 6.0]), [0.0, 1.5])
    d = fr.solve2([[1.0, 1.0], [1.0, 1.0]], [2.0, 2.0])                                        # rank 1, full matrix
    assert d[1] == 0.0 and abs(d[0] - 2.0) < 1e-14


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_known_shift_is_recovered(inverse, levels):
    a = fr.texture(160, 128, seed=11)
    b = fr.texture(160, 128, seed=11, shift=SHIFT)
    pts = np.array([(x, y) for y in range(40, 100, 16) for x in range(40, 130, 20)], dtype=np.float32)
    out, st, its, cost = fr.multi_level(a, b, pts, levels=levels, inverse=inverse)
    assert np.all(st == fr.OK)
    err = np.max(np.linalg.norm(out - pts - np.array([-SHIFT[0], -SHIFT[1]], dtype=np.float32), axis=1))
    print("levels %d inverse %d: worst error %.4f px" % (levels, inverse, err))
    assert err <= SHIFT_BAR, err


@pytest.mark.parametrize("inverse", [0, 1])
def test_flat_image_gives_no_step_and_the_references_statuses(inverse):
    """H is rank 0, dp = 0: the position stays and, the cost never rising above DBL_MAX, every step counts as taken (tracked)."""
    a = np.full((48, 64), 90, dtype=np.uint8)
    pts = np.array([[20.5, 20.25], [2.0, 20.0]], dtype=np.float32)
    out, st, its, cost = fr.multi_level(a, a, pts, levels=2, inverse=inverse)
    assert np.array_equal(out, pts)
    assert list(st) == [fr.OK, fr.FAIL_LOST] and list(its) == [10, 0] and cost[0] == 0.0 and np.isnan(cost[1])
    out, st, its, cost = fr.multi_level(a, a, pts, levels=2, inverse=inverse, early_stop=1)
    assert np.array_equal(out, pts) and list(st) == [fr.OK, fr.FAIL_LOST] and list(its) == [2, 0]


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("half_patch", [4, 10])
def test_fixture_pair_is_the_same_in_both_orders(inverse, half_patch):
    """All 170 keypoints track, and adding the patch's terms in the wave's order instead of the loop's changes no output float,
    iteration count or status (the cap of tests/test_gpu_flow.py allows the device 2 %)."""
    im1, im2, kp = fixture_pair()
    assert im1.shape == (480, 752) and len(kp) == 170
    seq = fr.multi_level(im1, im2, kp, inverse=inverse, half_patch=half_patch, order="sequential")
    wav = fr.multi_level(im1, im2, kp, inverse=inverse, half_patch=half_patch, order="wave64")
    assert np.all(seq[1] == fr.OK) and np.all(wav[1] == fr.OK)
    flow = np.median(np.linalg.norm(seq[0] - kp, axis=1))
    print("inverse %d half_patch %d: median flow %.3f px" % (inverse, half_patch, flow))
    assert 7.0 < flow < 8.5
    assert np.array_equal(seq[0].view(np.uint32), wav[0].view(np.uint32)) and np.array_equal(seq[2], wav[2])
