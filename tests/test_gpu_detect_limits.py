"""The batched corner detector on the GPU (include/vio_detect.h) where its two greedy loops have more entries than threads: setMask
over 255 to 4096 tracked points (k_detect_setmask has 256 threads: from 257 points on a thread owns several entries and strikes them
across rounds) and the selection over 1023 to 2049 candidates (k_detect_select has 1024 threads), against the numpy restatement
(tests/detect_reference.py) under same() of tests/test_gpu_detect.py: every count, keep_order and new_pts exact, no tolerance.  The
images are uniform noise.  Each case asserts on the reference that the sizes it names were reached.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import front_limits_inputs as fl  # noqa: E402
from test_gpu_detect import random_image, result_bytes, same  # noqa: E402

pytestmark = pytest.mark.gpu
NT_MASK, NT_SEL, MAX_POINTS = 256, 1024, 4096
TW, TH = 129, 97                                        # the image of the tracked-point cases
CW, CH = 224, 168                                       # ... and of the candidate cases
_cache = {}


@pytest.fixture(scope="module")
def detect_lib(vio, hip_lib):
    return vio.load_detect()


@pytest.fixture()
def dh(detect_lib):
    h = detect_lib.create()
    yield h
    h.close()


def noise(w, h):
    if (w, h) not in _cache:
        img = random_image(w, h)
        _cache[(w, h)] = (img, dr.response(img))
    return _cache[(w, h)]


def tracked_points(n, w=TW, h=TH):
    rng = np.random.RandomState(1000 + n)
    return np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)


def tie_counts(n):
    return np.random.RandomState(n).randint(1, 4, size=n).astype(np.int32)


def reference(name, img, R, tracked, cnt, mask, max_total, min_distance):
    """The restatement's result, computed once per name (the greedy over 4096 points takes it seconds)."""
    if ("ref", name) not in _cache:
        _cache[("ref", name)] = dr.detect(img, tracked, cnt, mask, max_total, min_distance=min_distance, R=R)
    return _cache[("ref", name)]


def run(dh, img, R, tracked, cnt, mask, max_total, min_distance, name):
    dh.set_config(min_distance=min_distance)
    got = dh.detect(img, tracked, cnt, mask, max_total)
    ref = reference(name, img, R, tracked, cnt, mask, max_total, min_distance)
    same(got, ref, name)
    return got, ref


# ---- tracked points across NT_MASK -------------------------------------------------------------------------------
TRACKED = [(n, d) for n in (255, 256, 257, 511, 1024) for d in (0, 1, 3)] + [(MAX_POINTS, 3)]


@pytest.mark.parametrize("counts", ["ties", "equal"])
@pytest.mark.parametrize("n,min_distance", TRACKED)
def test_tracked_points(dh, n, min_distance, counts):
    """Counts from randint(1, 4): many ties, the index decides among them; every count equal: the index decides everything."""
    img, R = noise(TW, TH)
    pts = tracked_points(n)
    cnt = tie_counts(n) if counts == "ties" else np.full(n, 3, np.int32)
    got, ref = run(dh, img, R, pts, cnt, None, MAX_POINTS, min_distance, "%d tracked d%d %s" % (n, min_distance, counts))
    if n >= 2 * NT_MASK - 1:
        assert ref["n_kept"] > NT_MASK, ref["n_kept"]                   # more rounds than threads, more winners than threads
    if min_distance >= 1:
        assert ref["n_kept"] != n                                       # something was struck
    if counts == "equal" and min_distance == 0:
        assert np.all(np.diff(ref["keep_order"]) > 0)                   # the index alone


def test_tracked_points_on_zero_mask_pixels(dh):
    img, R = noise(TW, TH)
    n = 1024
    pts = tracked_points(n)
    closed = np.random.RandomState(3).choice(n, size=300, replace=False)
    c = dr.round_points(pts)
    mask = np.ones((TH, TW), dtype=np.uint8)
    mask[c[closed, 1], c[closed, 0]] = 0
    got, ref = run(dh, img, R, pts, tie_counts(n), mask, MAX_POINTS, 1, "300 of 1024 on zero mask pixels")
    assert NT_MASK < ref["n_kept"] <= n - 300 and not np.isin(closed, ref["keep_order"]).any()
    assert len(set((closed % NT_MASK).tolist())) > NT_MASK // 2         # struck from the start in most of the threads' lists


def test_every_tracked_point_and_nothing_wanted(dh):
    img, R = noise(TW, TH)
    pts = tracked_points(MAX_POINTS)
    got, ref = run(dh, img, R, pts, tie_counts(MAX_POINTS), None, 0, 3, "4096 tracked, max_total 0")
    assert ref["n_kept"] > NT_MASK and ref["n_new"] == 0 and got["n_new"] == 0 and len(got["new_pts"]) == 0


# ---- candidates across NT_SEL ------------------------------------------------------------------------------------
def candidate_mask(target):
    """A mask that closes pixels on surplus candidates of the noise image, never on the maximum: `target` candidates stay (closing a
    candidate's own pixel changes neither maxR nor any other candidate: a local maximum is one whatever the mask says)."""
    key = ("mask", target)
    if key not in _cache:
        img, R = noise(CW, CH)
        cand = dr.detect(img, max_total=0, min_distance=0, R=R)["candidates"]
        assert len(cand) > 2 * NT_SEL + 1, len(cand)
        best = cand[np.argmax(R.reshape(-1)[cand])]
        surplus = np.random.RandomState(target).permutation(cand[cand != best])[:len(cand) - target]
        mask = np.ones((CH, CW), dtype=np.uint8)
        mask.reshape(-1)[surplus] = 0
        assert mask.reshape(-1)[best] == 1
        _cache[key] = mask
    return _cache[key]


@pytest.mark.parametrize("min_distance", [0, 3])
@pytest.mark.parametrize("target", [NT_SEL - 1, NT_SEL, NT_SEL + 1, 2 * NT_SEL, 2 * NT_SEL + 1])
def test_candidates(dh, target, min_distance):
    img, R = noise(CW, CH)
    mask = candidate_mask(target)
    got, ref = run(dh, img, R, None, None, mask, MAX_POINTS, min_distance, "%d candidates d%d, all" % (target, min_distance))
    assert ref["n_candidates"] == target
    if min_distance == 0:
        assert ref["n_new"] == target                                   # every candidate is taken: more than 1024 where there are as many
    else:
        assert NT_SEL // 4 < ref["n_new"] < target                      # some are struck
    stop = ref["n_new"] // 2 + 1
    got2, ref2 = run(dh, img, R, None, None, mask, stop, min_distance, "%d candidates d%d, %d wanted" % (target, min_distance, stop))
    assert ref2["n_new"] == stop and ref2["n_candidates"] == target     # the rounds stop in mid-list
    assert got2["new_pts"].tobytes() == got["new_pts"][:stop].tobytes()


# ---- the batch ---------------------------------------------------------------------------------------------------
def test_batch_of_extremes(dh):
    (img_t, R_t), (img_c, R_c) = noise(TW, TH), noise(CW, CH)
    names = ["4096 tracked d3 ties", "2 x 2", "2049 candidates d3, all", "nothing tracked, nothing wanted"]      # (the first and the third: computed above)
    items = [dict(img=img_t, tracked=tracked_points(MAX_POINTS), track_cnt=tie_counts(MAX_POINTS), mask=None, max_total=MAX_POINTS),
             dict(img=random_image(2, 2), tracked=np.float32([[1.0, 0.0]]), track_cnt=[1], mask=None, max_total=5),
             dict(img=img_c, tracked=None, track_cnt=None, mask=candidate_mask(2 * NT_SEL + 1), max_total=MAX_POINTS),
             dict(img=img_t, tracked=None, track_cnt=None, mask=None, max_total=0)]
    dh.set_config(min_distance=3)
    outs = dh.detect_batch(items)
    again = dh.detect_batch(items)
    for i, (o, o2, it) in enumerate(zip(outs, again, items)):
        assert result_bytes(o) == result_bytes(o2), i
        R = {0: R_t, 2: R_c, 3: R_t}.get(i)
        same(o, reference(names[i], it["img"], R, it["tracked"], it["track_cnt"], it["mask"], it["max_total"], 3), "item %d" % i)
        assert result_bytes(dh.detect_batch([it])[0]) == result_bytes(o), i
    assert outs[0]["n_kept"] > NT_MASK and outs[1]["n_kept"] == 1 and outs[2]["n_candidates"] == 2 * NT_SEL + 1
    assert outs[3]["n_kept"] == outs[3]["n_new"] == 0 and outs[3]["n_candidates"] > 0


# ---- the resident path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [False, True])
def test_resident_frame_with_a_full_table(vio, dh, equalize):
    """FrameHandle.detect with 1024 tracked points on a 192 x 144 slot against DetectHandle.detect on the same level 0."""
    fr = vio.load_frame().create()
    try:
        fr.set_config(equalize=equalize, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow=dict(levels=2, half_patch=2), detect=dict(min_distance=fl.MIN_DIST))
        fr.push(fl.image(0), slot=200)
        pts, _, cnt = fl.seeded(fl.CAP)
        got = fr.detect(tracked=pts, track_cnt=cnt, max_total=fl.CAP, slot=200)
        level0 = fr.download(200, 1, 0)
        assert level0.shape == (fl.H, fl.W) and np.array_equal(level0, fl.image(0)) != equalize
        dh.set_config(min_distance=fl.MIN_DIST)
        ref = dh.detect(level0, pts, cnt, None, fl.CAP)
        same(got, ref, "resident, 1024 tracked")
        assert NT_MASK < ref["n_kept"] < fl.CAP and ref["n_new"] > 0 and not np.array_equal(ref["keep_order"], np.arange(ref["n_kept"]))
    finally:
        fr.close()
