"""numpy restatement of include/vio_clahe.h: contrast-limited adaptive histogram equalisation of 8-bit images, the contract the
device is held to.

    geometry(w, h, tiles, clip_limit)       step 1 and 2: the extension, the tile, the clip limit, lut_scale and the two inv_tile values
    source(img, g)                          the image the histograms are taken of (extended with BORDER_REFLECT_101 where it must be)
    tile_hists(img, g)                      [tiles_y][tiles_x][256] integer histograms
    clip_hists(hist, clip)                  step 3 in the closed form a thread that owns a bin uses
    luts_of(hist, g)                        step 4
    blend(img, luts, g)                     step 5: (the output bytes, res before rounding)
    apply(img, clip_limit, tiles)           the five steps: what vio_clahe_apply_batch returns for one item
    apply_scalar(img, clip_limit, tiles)    the same as a plain walk, pixel by pixel and bin by bin, with OpenCV's own redistribution loop

Histograms, clip and redistribution are integers; a LUT entry is one float32 product rounded to nearest-even; the blend is a fixed
sequence of float32 operations (numpy rounds every one of them to float32 and fuses none).  The two formulations check each other, and
the device is expected to agree with both in every byte.
"""
import os

import numpy as np

OK = 0
BINS = 256
MAX_DIM, MAX_TILES = 16384, 16
DEFAULT_CLIP_LIMIT, DEFAULT_TILES = 3.0, (8, 8)
F = np.float32


def reflect_index(n, n_ext):
    """The source index of positions 0 .. n_ext - 1 of an axis of n pixels under BORDER_REFLECT_101: period 2 (n - 1), 0 for n = 1."""
    i = np.arange(n_ext)
    if n == 1:
        return np.zeros(n_ext, dtype=np.int64)
    p = 2 * (n - 1)
    m = i % p
    return np.where(m < n, m, p - m)


def geometry(w, h, tiles=DEFAULT_TILES, clip_limit=DEFAULT_CLIP_LIMIT):
    tx, ty = int(tiles[0]), int(tiles[1])
    assert 1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM and 1 <= tx <= MAX_TILES and 1 <= ty <= MAX_TILES
    assert np.isfinite(clip_limit) and clip_limit >= 0
    ext = not (w % tx == 0 and h % ty == 0)
    w_ext = w + (tx - w % tx) if ext else w          # (a direction that divides still gets a whole tx: cv::copyMakeBorder as CLAHE calls it)
    h_ext = h + (ty - h % ty) if ext else h
    tile_w, tile_h = w_ext // tx, h_ext // ty
    area = tile_w * tile_h
    assert area < 2 ** 31
    clip = 0
    if clip_limit != 0:
        clip = max(int(min(float(clip_limit) * float(area) / 256.0, float(area))), 1)     # double, truncated; no bin exceeds area
    return dict(w=w, h=h, tiles_x=tx, tiles_y=ty, ext=ext, w_ext=w_ext, h_ext=h_ext, tile_w=tile_w, tile_h=tile_h, area=area, clip=clip,
                lut_scale=F(255) / F(area), inv_tile_w=F(1) / F(tile_w), inv_tile_h=F(1) / F(tile_h))


def source(img, g):
    if not g["ext"]:
        return img
    return img[np.ix_(reflect_index(g["h"], g["h_ext"]), reflect_index(g["w"], g["w_ext"]))]


def tile_hists(img, g):
    s = source(img, g)
    ty, tx = g["tiles_y"], g["tiles_x"]
    t = s.reshape(ty, g["tile_h"], tx, g["tile_w"]).transpose(0, 2, 1, 3).reshape(ty * tx, g["area"]).astype(np.int64)
    flat = (t + BINS * np.arange(ty * tx)[:, None]).reshape(-1)
    return np.bincount(flat, minlength=BINS * ty * tx).reshape(ty, tx, BINS)


def clip_hists(hist, clip):
    """Step 3 for every tile at once, the +1 of the residual in its closed form."""
    if clip <= 0:
        return hist.copy()
    excess = np.maximum(hist - clip, 0).sum(axis=-1, keepdims=True)
    out = np.minimum(hist, clip)
    batch = excess // BINS
    residual = excess - BINS * batch
    step = np.maximum(BINS // np.maximum(residual, 1), 1)
    b = np.arange(BINS)
    plus = (residual > 0) & (b % step == 0) & (b // step < residual)
    return out + batch + plus


def luts_of(hist, g):
    sums = np.cumsum(hist, axis=-1)
    assert int(sums.max()) < 2 ** 31
    v = np.rint(sums.astype(F) * g["lut_scale"])
    return np.clip(v, 0, 255).astype(np.uint8)


def axis_weights(n, inv_tile, tiles):
    """(t1, t2, a, a1) of step 5 for the positions 0 .. n - 1 of one axis."""
    tf = np.arange(n).astype(F) * inv_tile - F(0.5)
    t1 = np.floor(tf).astype(np.int64)
    a = tf - t1.astype(F)
    a1 = F(1) - a
    assert a.dtype == F and a1.dtype == F and int(t1.max()) <= tiles - 1 and int(t1.min()) >= -1
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def blend(img, luts, g):
    tx1, tx2, xa, xa1 = axis_weights(g["w"], g["inv_tile_w"], g["tiles_x"])
    ty1, ty2, ya, ya1 = axis_weights(g["h"], g["inv_tile_h"], g["tiles_y"])
    L = luts.astype(F)
    v = img.astype(np.int64)
    l11, l12 = L[ty1[:, None], tx1[None, :], v], L[ty1[:, None], tx2[None, :], v]
    l21, l22 = L[ty2[:, None], tx1[None, :], v], L[ty2[:, None], tx2[None, :], v]
    res = (l11 * xa1 + l12 * xa) * ya1[:, None] + (l21 * xa1 + l22 * xa) * ya[:, None]
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8), res


def apply(img, clip_limit=DEFAULT_CLIP_LIMIT, tiles=DEFAULT_TILES, full=False):
    """The equalised image; full=True: dict(out, luts, clip, tile_w, tile_h, hist (before clipping), res)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    g = geometry(img.shape[1], img.shape[0], tiles, clip_limit)
    hist = tile_hists(img, g)
    luts = luts_of(clip_hists(hist, g["clip"]), g)
    out, res = blend(img, luts, g)
    if not full:
        return out
    return dict(status=OK, out=out, luts=luts, clip=g["clip"], tile_w=g["tile_w"], tile_h=g["tile_h"], hist=hist, res=res)


def apply_scalar(img, clip_limit=DEFAULT_CLIP_LIMIT, tiles=DEFAULT_TILES):
    """Steps 1 to 5 as written, one pixel and one bin at a time: (out, luts).  For small images."""
    img = np.asarray(img)
    h, w = img.shape
    g = geometry(w, h, tiles, clip_limit)
    tx_n, ty_n, tw, th, clip = g["tiles_x"], g["tiles_y"], g["tile_w"], g["tile_h"], g["clip"]

    def refl(i, n):
        if n == 1:
            return 0
        p = 2 * (n - 1)
        m = i % p
        return m if m < n else p - m

    luts = np.zeros((ty_n, tx_n, BINS), dtype=np.uint8)
    for ty in range(ty_n):
        for tx in range(tx_n):
            hist = [0] * BINS
            for y in range(ty * th, (ty + 1) * th):
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[int(img[refl(y, h), refl(x, w)]) if g["ext"] else int(img[y, x])] += 1
            if clip > 0:
                excess = 0
                for i in range(BINS):
                    if hist[i] > clip:
                        excess += hist[i] - clip
                        hist[i] = clip
                batch = excess // BINS
                residual = excess - BINS * batch
                for i in range(BINS):
                    hist[i] += batch
                if residual > 0:
                    step = max(BINS // residual, 1)
                    i = 0
                    while i < BINS and residual > 0:                # OpenCV's loop; it may leave some residual undistributed
                        hist[i] += 1
                        i += step
                        residual -= 1
            s = 0
            for i in range(BINS):
                s += hist[i]
                luts[ty, tx, i] = min(max(int(np.rint(F(s) * g["lut_scale"])), 0), 255)
    out = np.zeros((h, w), dtype=np.uint8)

    def weights(p, inv, n):
        tf = F(p) * inv - F(0.5)
        t1 = int(np.floor(tf))
        a = tf - F(t1)
        return max(t1, 0), min(t1 + 1, n - 1), a, F(1) - a

    for y in range(h):
        ty1, ty2, ya, ya1 = weights(y, g["inv_tile_h"], ty_n)
        for x in range(w):
            tx1, tx2, xa, xa1 = weights(x, g["inv_tile_w"], tx_n)
            v = int(img[y, x])
            res = (F(luts[ty1, tx1, v]) * xa1 + F(luts[ty1, tx2, v]) * xa) * ya1 + (F(luts[ty2, tx1, v]) * xa1 + F(luts[ty2, tx2, v]) * xa) * ya
            assert type(res) is F
            out[y, x] = min(max(int(np.rint(res)), 0), 255)
    return out, luts


class Equalizer:
    """The restatement behind ClaheHandle's interface (for frontend.FeatureTracker)."""

    def __init__(self, clip_limit=DEFAULT_CLIP_LIMIT, tiles=DEFAULT_TILES):
        self.cfg = dict(clip_limit=clip_limit, tiles=tiles)

    def set_config(self, clip_limit=DEFAULT_CLIP_LIMIT, tiles=DEFAULT_TILES):
        self.cfg = dict(clip_limit=clip_limit, tiles=tiles)

    def apply(self, img):
        return apply(img, **self.cfg)


# ---------------------------------------------------------------------------------------------------------
# the cases the host mirror and the GPU are held to (tests/test_clahe_host_mirror.py, tests/test_gpu_clahe.py)
# ---------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_SHAPES = [(1, 1), (2, 5), (5, 2), (7, 9), (8, 8), (16, 16), (17, 13), (16, 13), (13, 16)]       # (width, height)


def random_image(w, h, seed=7):
    return np.random.RandomState(seed + 131 * w + h).randint(0, 256, size=(h, w)).astype(np.uint8)


def two_valued(w, h, seed=3):
    return np.where(np.random.RandomState(seed).uniform(size=(h, w)) < 0.3, 20, 230).astype(np.uint8)


def smooth(w, h):
    """A ramp with a little texture: neighbouring tiles have different, well filled histograms."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 3 + yy * 5 + 40 * np.sin(xx / 7.0) * np.cos(yy / 5.0)) % 256).astype(np.uint8)


def fixture_image():
    return np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]


def tile_shapes(TX, TY):
    """Every combination of T - 1, T, T + 1, 2 T + 1 per direction for the apply kernel's pixel tile."""
    return [(w, h) for w in (TX - 1, TX, TX + 1, 2 * TX + 1) for h in (TY - 1, TY, TY + 1, 2 * TY + 1)]


def config_cases():
    """(name, image, clip_limit, tiles) besides the shapes: the tile grids, the clip limits, the kinds of image."""
    out = []
    for tiles in ((1, 1), (3, 5), (16, 16)):
        for (w, h) in ((37, 29), (48, 80), (1, 1)):
            out.append(("tiles %dx%d %dx%d" % (tiles + (w, h)), random_image(w, h, seed=11), 3.0, tiles))
    for cl in (0.0, 1e-3, 3.0, 40.0):
        out.append(("clip %g random" % cl, random_image(61, 45, seed=5), cl, (8, 8)))
        out.append(("clip %g smooth" % cl, smooth(96, 72), cl, (8, 8)))
        out.append(("clip %g flat" % cl, np.full((33, 41), 77, dtype=np.uint8), cl, (8, 8)))
        out.append(("clip %g two-valued" % cl, two_valued(70, 50), cl, (8, 8)))
    # a tile of 100 x 70 = 7000 > 256 * 4 pixels: every thread of the histogram loops; 3 x 2 tiles, not a multiple in y
    out.append(("large tile", smooth(300, 139), 3.0, (3, 2)))
    return out
