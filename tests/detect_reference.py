"""numpy restatement of include/vio_detect.h: setMask and Shi-Tomasi corner detection, the contract the device is held to (DESIGN.md
section 20).

    sobel(img)                              the 3 x 3 Sobel pair with BORDER_REFLECT_101: integers
    box_sums(img)                           a, b, c: the 3 x 3 box sums of the product maps, again BORDER_REFLECT_101: integers
    response(img)                           R = 0.5 ((a + c) - sqrt((a - c)^2 + 4 b^2)): one sqrt of an exact operand
    set_mask(...)                           the kept tracked points, in output order
    candidates(...)                         the candidate pixels and maxR
    select(...)                             the serial greedy over the sorted candidates
    detect(...)                             the four steps: what vio_detect_batch returns for one item

Every quantity is an integer up to the one correctly rounded square root, so the device is expected to agree in every bit.  The selection
here walks the sorted list and compares with every corner accepted so far; the device repeatedly takes the best remaining candidate and
strikes its neighbours.  The two formulations check each other.
"""
import numpy as np

OK, NOT_FINITE = 0, -3
MAX_DIM, MAX_POINTS = 16384, 4096
BLOCK, APERTURE = 3, 3
DEFAULT_QUALITY, DEFAULT_MIN_DISTANCE, DEFAULT_MAX_TOTAL = 0.01, 30, 150


def _refl(n):
    """The indices of positions -1 .. n under BORDER_REFLECT_101 (a one-pixel axis repeats its pixel)."""
    i = np.abs(np.arange(-1, n + 1))
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)


def _pad(a):
    return a[np.ix_(_refl(a.shape[0]), _refl(a.shape[1]))]


def sobel(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    p = _pad(img.astype(np.int64))
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return gx, gy


def _box(a):
    p = _pad(a)
    h, w = a.shape
    return sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3))


def box_sums(img):
    gx, gy = sobel(img)
    return _box(gx * gx), _box(gx * gy), _box(gy * gy)


def radicand(a, b, c):
    return (a - c) ** 2 + 4 * b * b


def response(img):
    a, b, c = box_sums(img)
    rad = radicand(a, b, c)
    assert int(rad.max()) < 2 ** 53 and int(a.max()) < 2 ** 31 and int(c.max()) < 2 ** 31
    return 0.5 * ((a + c).astype(np.float64) - np.sqrt(rad.astype(np.float64)))


def round_points(pts):
    """cvRound of the float positions: ties to even."""
    return np.rint(np.asarray(pts, dtype=np.float32).reshape(-1, 2).astype(np.float64)).astype(np.int64)


def set_mask(shape, tracked, track_cnt, mask=None, min_distance=DEFAULT_MIN_DISTANCE):
    """(keep_order, allowed): the indices of the kept points in output order, and the map of allowed pixels."""
    h, w = shape
    allowed = np.ones((h, w), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    allowed = allowed.copy()
    c = round_points(tracked)
    cnt = np.asarray(track_cnt, dtype=np.int64).reshape(-1)
    assert len(cnt) == len(c)
    assert np.all((c[:, 0] >= 0) & (c[:, 0] < w) & (c[:, 1] >= 0) & (c[:, 1] < h)), "a tracked point rounds to a pixel outside the image"
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = int(min_distance) ** 2
    keep = []
    for i in sorted(range(len(c)), key=lambda k: (-int(cnt[k]), k)):
        x, y = int(c[i, 0]), int(c[i, 1])
        if mask is not None and mask[y, x] == 0:
            continue
        if any((x - int(c[j, 0])) ** 2 + (y - int(c[j, 1])) ** 2 <= d2 for j in keep):
            continue
        keep.append(i)
        allowed &= ~((xx - x) ** 2 + (yy - y) ** 2 <= d2)
    return np.array(keep, dtype=np.int32), allowed


def candidates(R, allowed, quality=DEFAULT_QUALITY):
    """(the candidates' pixel indices y W + x ascending, maxR)."""
    h, w = R.shape
    max_r = float(R[allowed].max()) if allowed.any() else 0.0
    if h < 3 or w < 3:
        return np.zeros(0, dtype=np.int64), max_r
    t = max_r * quality
    c = R[1:-1, 1:-1]
    ok = allowed[1:-1, 1:-1] & (c > t) & (c > 0)
    for dj in range(3):
        for di in range(3):
            ok &= c >= R[dj:dj + h - 2, di:di + w - 2]
    ys, xs = np.nonzero(ok)
    return (ys + 1) * w + (xs + 1), max_r


def select(R, cand, n_want, min_distance=DEFAULT_MIN_DISTANCE):
    """The serial greedy over the candidates in the order (R descending, pixel index descending): (n, 2) float32 (x, y)."""
    w = R.shape[1]
    out = []
    if n_want <= 0 or len(cand) == 0:
        return np.zeros((0, 2), dtype=np.float32)
    order = np.lexsort((cand, R.reshape(-1)[cand]))[::-1]
    d2 = int(min_distance) ** 2
    acc = np.zeros((0, 2), dtype=np.int64)
    for p in cand[order]:
        x, y = int(p % w), int(p // w)
        if len(acc) and np.any((acc[:, 0] - x) ** 2 + (acc[:, 1] - y) ** 2 < d2):
            continue
        acc = np.concatenate([acc, [[x, y]]])
        out.append((x, y))
        if len(out) >= n_want:
            break
    return np.array(out, dtype=np.float32).reshape(-1, 2)


def detect(img, tracked=None, track_cnt=None, mask=None, max_total=DEFAULT_MAX_TOTAL, quality=DEFAULT_QUALITY,
           min_distance=DEFAULT_MIN_DISTANCE, R=None):
    """What vio_detect_batch returns for one item (R: the image's response map if the caller has it already)."""
    img = np.asarray(img)
    pts = np.zeros((0, 2), dtype=np.float32) if tracked is None else np.asarray(tracked, dtype=np.float32).reshape(-1, 2)
    cnt = np.ones(len(pts), dtype=np.int32) if track_cnt is None else np.asarray(track_cnt, dtype=np.int32).reshape(-1)
    if not np.all(np.isfinite(pts)):
        return dict(status=NOT_FINITE, n_kept=0, n_new=0, n_candidates=0, max_response=0.0, keep_order=np.zeros(0, dtype=np.int32),
                    new_pts=np.zeros((0, 2), dtype=np.float32))
    keep, allowed = set_mask(img.shape, pts, cnt, mask, min_distance)
    R = response(img) if R is None else R
    cand, max_r = candidates(R, allowed, quality)
    new = select(R, cand, int(max_total) - len(keep), min_distance)
    return dict(status=OK, n_kept=len(keep), n_new=len(new), n_candidates=len(cand), max_response=max_r, keep_order=keep, new_pts=new,
                candidates=cand)


class Detector:
    """The restatement behind DetectHandle's interface (for frontend.FeatureTracker)."""

    def __init__(self):
        self.cfg = dict(quality=DEFAULT_QUALITY, min_distance=DEFAULT_MIN_DISTANCE)

    def set_config(self, quality=DEFAULT_QUALITY, min_distance=DEFAULT_MIN_DISTANCE):
        self.cfg = dict(quality=quality, min_distance=min_distance)

    def detect(self, img, tracked=None, track_cnt=None, mask=None, max_total=DEFAULT_MAX_TOTAL):
        return detect(img, tracked, track_cnt, mask, max_total, **self.cfg)
