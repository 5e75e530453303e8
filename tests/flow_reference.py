"""numpy restatement of include/vio_flow.h: the pyramidal Lucas-Kanade tracker the device is held to.

    pyr_down(img)                         cv::pyrDown of an 8-bit image to (W / 2, H / 2): integers, exact
    pyramid(img, levels)                  the levels, level 0 first
    scharr(img)                           cv::Scharr(CV_64F) in x and in y, BORDER_REFLECT_101: integers
    solve2(H, b)                          Eigen 3.3's H.fullPivHouseholderQr().solve(b) for 2 x 2
    single_level(...)                     OpticalFlowSingleLevel for one keypoint
    multi_level(...)                      OpticalFlowMultiLevel for many

order="sequential" adds the patch's terms in the reference's loop order; order="wave64" adds them as the header's order contract says
(pixel m to lane m mod 64, each lane ascending from 0.0, then the butterfly v[i] += v[i ^ s], s = 1 .. 32).  Every product and sum
is one rounded double operation (numpy does not contract), positions are float at the level boundaries.
"""
import numpy as np

OK, NOT_FINITE = 0, -3
FAIL_LOST, FAIL_BORDER = 1, 2
MAX_LEVELS, MAX_HALF_PATCH, MAX_POINTS = 8, 16, 4096
DEFAULT_CFG = dict(levels=4, half_patch=4, max_iter=10, inverse=0, border=1, early_stop=0)
GRADIENT_DIVISOR = 26.0
EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)
DBL_MAX = float(np.finfo(np.float64).max)
_K5 = (1, 4, 6, 4, 1)
_LANE = np.arange(64)


def pyr_down(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    oh, ow = h // 2, w // 2
    p = np.pad(img.astype(np.int32), 2, mode="reflect")
    rows = sum(k * p[:, i:i + 2 * ow:2] for i, k in enumerate(_K5))
    out = sum(k * rows[i:i + 2 * oh:2, :] for i, k in enumerate(_K5))
    return ((out + 128) >> 8).astype(np.uint8)


def level_sizes(width, height, levels):
    out = [(int(width), int(height))]
    for _ in range(levels - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


def scharr(img):
    p = np.pad(np.asarray(img).astype(np.int32), 1, mode="reflect")
    gx = 3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])
    gy = 3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])
    return gx.astype(np.float64), gy.astype(np.float64)


def solve2(H, b):
    """FullPivHouseholderQR<Matrix2d>::compute and _solve_impl of Eigen 3.3, restated: the largest |entry| (the first in column-major
    order) to the corner, one Householder reflection, the rank from the threshold 2 eps, the basic solution."""
    m = [[float(H[0][0]), float(H[0][1])], [float(H[1][0]), float(H[1][1])]]
    prec = EPS * 2.0
    r, c, best = 0, 0, abs(m[0][0])
    for (i, j) in ((1, 0), (0, 1), (1, 1)):
        if abs(m[i][j]) > best:
            r, c, best = i, j, abs(m[i][j])
    biggest = best
    if best <= biggest * prec:                          # (zero matrix: rank 0)
        return np.zeros(2)
    if r != 0:
        m[0], m[1] = m[1], m[0]
    if c != 0:
        m[0][0], m[0][1] = m[0][1], m[0][0]
        m[1][0], m[1][1] = m[1][1], m[1][0]
    tail2 = m[1][0] * m[1][0]
    c0 = m[0][0]
    if tail2 <= TINY:
        tau, beta, ess = 0.0, c0, 0.0
    else:
        beta = float(np.sqrt(c0 * c0 + tail2))
        if c0 >= 0:
            beta = -beta
        ess = m[1][0] / (c0 - beta)
        tau = (beta - c0) / beta
    m[0][0] = beta
    maxpivot = abs(beta)
    if tau != 0.0:
        tmp = ess * m[1][1]
        tmp = tmp + m[0][1]
        m[0][1] = m[0][1] - tau * tmp
        m[1][1] = m[1][1] - (tau * ess) * tmp
    nonzero = 2
    if abs(m[1][1]) <= biggest * prec:
        nonzero = 1
    elif abs(m[1][1]) > maxpivot:
        maxpivot = abs(m[1][1])
    thr = maxpivot * prec
    diag = (m[0][0], m[1][1])
    rank = sum(1 for i in range(nonzero) if abs(diag[i]) > thr)
    if rank == 0:
        return np.zeros(2)
    cv = [float(b[0]), float(b[1])]
    if r != 0:
        cv[0], cv[1] = cv[1], cv[0]
    if tau != 0.0:
        tmp = ess * cv[1]
        tmp = tmp + cv[0]
        cv[0] = cv[0] - tau * tmp
        cv[1] = cv[1] - (tau * ess) * tmp
    with np.errstate(all="ignore"):
        if rank == 2:
            cv[1] = float(np.float64(cv[1]) / np.float64(m[1][1]))
            cv[0] = cv[0] - cv[1] * m[0][1]
            cv[0] = float(np.float64(cv[0]) / np.float64(m[0][0]))
        else:
            cv[0] = float(np.float64(cv[0]) / np.float64(m[0][0]))
            cv[1] = 0.0
    out = np.zeros(2)
    out[c] = cv[0]
    out[1 - c] = cv[1]
    return out


def is_valid_patch(x, y, w, h, hp):
    """IsValidPatch with int() truncation: hp <= int(x), int(x) + 1 <= w - hp, restated on the doubles (the same for every finite x)."""
    return bool(hp <= x < w - hp and hp <= y < h - hp)


def _bilinear(arr, x, y):
    """GetPixelValue / GetGradient (before the division) at the arrays x, y of non-negative doubles; x1, y1 are clamped to the image
    (where the clamp acts, their weight is exactly 0)."""
    h, w = arr.shape
    x0 = x.astype(np.int64)
    y0 = y.astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    xx = x - x0
    yy = y - y0
    return ((1 - xx) * (1 - yy) * arr[y0, x0] + xx * (1 - yy) * arr[y0, x1] + (1 - xx) * yy * arr[y1, x0] + xx * yy * arr[y1, x1])


def _sum(terms, order):
    """The sums of the rows of terms (k, n) in the order asked for."""
    k, n = terms.shape
    if order == "sequential":
        return np.cumsum(np.concatenate([np.zeros((k, 1)), terms], axis=1), axis=1)[:, -1]
    assert order == "wave64"
    per = (n + 63) // 64
    pad = np.zeros((k, per * 64))
    pad[:, :n] = terms                                  # (a lane's missing terms: + 0.0 changes nothing)
    v = np.cumsum(np.concatenate([np.zeros((k, 1, 64)), pad.reshape(k, per, 64)], axis=1), axis=1)[:, -1, :]
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, _LANE ^ s]
    return v[:, 0]


class Level:
    """An image level with its Scharr gradients (ImageWithGradient)."""

    def __init__(self, img):
        self.img = np.asarray(img).astype(np.float64)
        self.h, self.w = self.img.shape
        self.gx, self.gy = scharr(img)


def single_level(T, I, x0, y0, dx, dy, half_patch=4, max_iter=10, inverse=False, order="sequential", early_stop=False):
    """OpticalFlowSingleLevel for one keypoint: T, I are Levels, (x0, y0) the keypoint in T, (dx, dy) the start.  Returns (dx, dy,
    success, iterations evaluated, the last evaluated cost or NaN)."""
    hp = int(half_patch)
    success, its, last_cost, cost_prev = False, 0, np.nan, DBL_MAX
    if not is_valid_patch(x0, y0, T.w, T.h, hp):
        return dx, dy, success, its, last_cost
    m = np.arange(4 * hp * hp)
    du = (m // (2 * hp) - hp).astype(np.float64)
    dv = (m % (2 * hp) - hp).astype(np.float64)
    tx, ty = x0 + du, y0 + dv
    tval = _bilinear(T.img, tx, ty)
    if inverse:
        jx = _bilinear(T.gx, tx, ty) / GRADIENT_DIVISOR
        jy = _bilinear(T.gy, tx, ty) / GRADIENT_DIVISOR
        hs = None
    for _ in range(int(max_iter)):
        x, y = x0 + dx, y0 + dy
        if not is_valid_patch(x, y, I.w, I.h, hp):
            success = False
            break
        ix, iy = x + du, y + dv
        err = tval - _bilinear(I.img, ix, iy)
        if not inverse:
            jx = _bilinear(I.gx, ix, iy) / GRADIENT_DIVISOR
            jy = _bilinear(I.gy, ix, iy) / GRADIENT_DIVISOR
            s = _sum(np.stack([jx * jx, jx * jy, jy * jy, err * jx, err * jy, 0.5 * err * err]), order)
            hs = s[:3]
        else:
            if hs is None:
                hs = _sum(np.stack([jx * jx, jx * jy, jy * jy]), order)
            s = np.concatenate([hs, _sum(np.stack([err * jx, err * jy, 0.5 * err * err]), order)])
        dp = solve2([[hs[0], hs[1]], [hs[1], hs[2]]], s[3:5])
        cost = float(s[5])
        its += 1
        last_cost = cost
        if np.isnan(dp[0]) or np.isnan(dp[1]):
            success = False
            break
        if cost_prev <= cost:
            break
        if early_stop:
            cost_prev = cost
        dx = dx + float(dp[0])
        dy = dy + float(dp[1])
        success = True
    return dx, dy, success, its, last_cost


def multi_level(img1, img2, pts, guess=None, levels=4, half_patch=4, max_iter=10, inverse=0, border=1, early_stop=0,
                order="sequential"):
    """OpticalFlowMultiLevel and readImage's border test: (next_pts (n, 2) float32, status (n,), iterations (n,), cost (n,))."""
    f32 = np.float32
    pts = np.asarray(pts, dtype=f32).reshape(-1, 2)
    n = len(pts)
    guess = None if guess is None else np.asarray(guess, dtype=f32).reshape(-1, 2)
    p1 = [Level(a) for a in pyramid(img1, levels)]
    p2 = [Level(a) for a in pyramid(img2, levels)]
    h0, w0 = p1[0].img.shape
    out = np.full((n, 2), np.nan, dtype=f32)
    status = np.zeros(n, dtype=np.int32)
    iters = np.zeros(n, dtype=np.int32)
    cost = np.full(n, np.nan)
    for i in range(n):
        if not np.all(np.isfinite(pts[i])) or (guess is not None and not np.all(np.isfinite(guess[i]))):
            status[i] = NOT_FINITE
            continue
        src = None
        for l in range(levels - 1, -1, -1):
            scale = 0.5 ** l
            tgt = (f32(np.float64(pts[i, 0]) * scale), f32(np.float64(pts[i, 1]) * scale))
            if l == levels - 1:
                src = tgt if guess is None else (f32(np.float64(guess[i, 0]) * scale), f32(np.float64(guess[i, 1]) * scale))
            x0, y0 = float(tgt[0]), float(tgt[1])
            dx, dy = float(src[0]) - x0, float(src[1]) - y0
            dx, dy, ok, its, c = single_level(p1[l], p2[l], x0, y0, dx, dy, half_patch, max_iter, bool(inverse), order, bool(early_stop))
            with np.errstate(over="ignore"):
                src = (f32(tgt[0] + f32(dx)), f32(tgt[1] + f32(dy)))
                if l > 0:
                    src = (f32(np.float64(src[0]) / 0.5), f32(np.float64(src[1]) / 0.5))
        out[i] = src
        iters[i], cost[i] = its, c
        if not ok:
            status[i] = FAIL_LOST
        else:
            with np.errstate(invalid="ignore"):
                rx, ry = np.rint(np.float64(src[0])), np.rint(np.float64(src[1]))
            inside = border <= rx < w0 - border and border <= ry < h0 - border
            status[i] = OK if inside else FAIL_BORDER
    return out, status, iters, cost


def texture(width, height, seed, shift=(0.0, 0.0), smooth=3.0):
    """A smooth seeded texture as uint8, sampled at (x + shift[0], y + shift[1]): a sum of low-frequency sinusoids, so that the
    shifted image is the same function sampled elsewhere."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    xx = xx + shift[0]
    yy = yy + shift[1]
    img = np.zeros((height, width))
    for _ in range(24):
        fx, fy = rng.uniform(-1, 1, 2) * (2 * np.pi / (4.0 * smooth))
        img += rng.uniform(0.3, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 2 * np.pi))
    img = 128.0 + 110.0 * img / 6.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
