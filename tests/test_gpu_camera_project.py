"""vio_camera_project_batch and vio_camera_set_inv_poly on the GPU (include/vio_camera_project.h, k_camera_project)
against tests/camera_project_reference.py: pixels and flags byte for byte, no tolerance.  All four models, with and without
distortion; 0 to 4096 points; four items of four models in one call, each equal to the item alone and to the call again; one camera in
two slot numbers; flagged points among good ones; inv_poly of 1 and 20 coefficients, missing, and cleared by vio_camera_set; the
argument rules; and vio_camera_lift_batch on the same handle before and after the new calls, against its own restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_project_reference as cp  # noqa: E402
import camera_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG, NOT_FINITE_STATUS = -1, cr.NOT_FINITE
PLAIN = dict(model=cr.MODEL_PINHOLE, width=752, height=480, fx=460.0, fy=459.5, cx=376.0, cy=240.0)
SLOTS = {0: cr.EUROC, 1: cr.KB_FOUR, 2: cr.MEI, 3: cr.SCARAMUZZA, 4: cr.MEI_PLAIN, 5: PLAIN, 6: cr.KB_ZERO, 7: cr.KB_CURVED}
NS = [0, 1, 63, 64, 65, 257, 4096]
_cache = {}


def ref_cam(params):
    key = tuple(sorted(params.items()))
    if key not in _cache:
        _cache[key] = cr.Camera(**params)
    return _cache[key]


def inv_of(params):
    cam = ref_cam(params)
    key = ("inv",) + tuple(sorted(params.items()))
    if cam.model != cr.MODEL_SCARAMUZZA:
        return None
    if key not in _cache:
        _cache[key] = cp.fit_inv_poly(cam)
    return _cache[key]


@pytest.fixture(scope="module")
def lib(vio, hip_lib):
    return vio.load_camera()


@pytest.fixture()
def ch(lib):
    h = lib.create()
    for s, p in SLOTS.items():
        h.set_camera(slot=s, **p)
        if inv_of(p) is not None:
            h.set_inv_poly(s, inv_of(p))
    yield h
    h.close()


def points(n, seed=0):
    """n points in front of the camera, up to 60 degrees off the axis, 0.5 to 25 deep."""
    rng = np.random.RandomState(300 + seed + 7 * n)
    th, ph = rng.uniform(0.0, 1.05, n), rng.uniform(-np.pi, np.pi, n)
    d = rng.uniform(0.5, 25.0, n)
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1) * d[:, None]


def want(params, P, inv="fit"):
    pix, flags = cp.project(ref_cam(params), P, inv_of(params) if isinstance(inv, str) else inv)
    return pix, flags


def same(out, params, P, name, inv="fit"):
    pix, flags = want(params, P, inv)
    assert out["pixels"].shape == pix.shape and out["flags"].shape == flags.shape, name
    assert np.array_equal(out["flags"], flags), (name, "flags")
    assert out["pixels"].tobytes() == pix.tobytes(), (name, "%d of %d pixels differ" % (int(np.sum(out["pixels"] != pix)), pix.size))
    assert out["n_flagged"] == int(np.sum(flags != 0)), name
    assert out["status"] == (NOT_FINITE_STATUS if np.any(flags & cp.NOT_FINITE) else 0), name


def out_bytes(o):
    return (o["status"], o["n_flagged"], o["pixels"].tobytes(), o["flags"].tobytes())


@pytest.mark.parametrize("n", NS)
def test_every_model_and_size_against_the_restatement(ch, n):
    for slot, params in SLOTS.items():
        P = points(n, slot)
        out = ch.project_batch([dict(points=P, slot=slot)])[0]
        same(out, params, P, "slot %d n %d" % (slot, n))
        if n >= 63:
            assert out["n_flagged"] == 0 and np.all(np.isfinite(out["pixels"]))
    if n == 257:                                            # the pixels are where the camera sees the points: inside a generous frame
        out = ch.project(points(n, 0)[:, :] * [0.3, 0.3, 1.0], slot=5)
        assert np.all(np.abs(out - [376.0, 240.0]) < 460.0)


def test_four_items_of_four_models_in_one_call(ch):
    items = [dict(points=points(5, 1), slot=0), dict(points=points(0, 2), slot=1), dict(points=points(64, 3), slot=2), dict(points=points(130, 4), slot=3)]
    outs = ch.project_batch(items)
    assert [len(o["pixels"]) for o in outs] == [5, 0, 64, 130]
    for it, o in zip(items, outs):
        same(o, SLOTS[it["slot"]], it["points"], "item on slot %d" % it["slot"])
        alone = ch.project_batch([it])[0]
        assert out_bytes(alone) == out_bytes(o), it["slot"]
    again = ch.project_batch(items)
    assert [out_bytes(o) for o in again] == [out_bytes(o) for o in outs]
    back = ch.project_batch(items[::-1])[::-1]
    assert [out_bytes(o) for o in back] == [out_bytes(o) for o in outs]


def test_one_camera_in_two_slot_numbers(ch):
    for src, dst in ((0, 200), (1, 255), (3, 77)):
        ch.set_camera(slot=dst, **SLOTS[src])
        if inv_of(SLOTS[src]) is not None:
            ch.set_inv_poly(dst, inv_of(SLOTS[src]))
        P = points(130, dst)
        a, b = ch.project_batch([dict(points=P, slot=src), dict(points=P, slot=dst)])
        assert out_bytes(a) == out_bytes(b)


def test_flagged_points_among_good_ones(ch):
    for slot, params in SLOTS.items():
        P = points(70, 50 + slot)
        P[3] = [0.4, -0.2, -1.5]                            # behind
        P[10] = [0.0, 0.0, 2.0]                             # on the axis
        P[40] = [np.nan, 0.3, 2.0]
        P[64] = [0.1, 0.2, 0.0]                             # in the image plane
        P[65] = [0.1, np.inf, 1.0]
        out = ch.project_batch([dict(points=P, slot=slot)])[0]
        same(out, params, P, "flags slot %d" % slot)
        model = params["model"]
        f = out["flags"]
        assert f[40] & cp.NOT_FINITE and f[65] & cp.NOT_FINITE and np.all(np.isnan(out["pixels"][[40, 65]]))
        if model == cr.MODEL_PINHOLE:
            assert f[3] == cp.BEHIND and f[10] == 0 and f[64] == (cp.BEHIND | cp.NOT_FINITE) and np.all(np.isfinite(out["pixels"][3]))
        if model == cr.MODEL_SCARAMUZZA:
            assert f[10] == cp.NOT_FINITE and f[3] == 0
        if model == cr.MODEL_KANNALA_BRANDT:
            assert f[3] == 0 and f[10] == 0 and f[64] == 0
        good = np.ones(70, dtype=bool)
        good[[3, 10, 40, 64, 65]] = False
        clean = points(70, 50 + slot)
        ref = ch.project_batch([dict(points=clean, slot=slot)])[0]
        assert out["pixels"][good].tobytes() == ref["pixels"][good].tobytes() and not f[good].any()      # the neighbours are untouched
        assert out["status"] == NOT_FINITE_STATUS
    # a flagged item does not touch the other items of its call
    P, bad = points(65, 9), points(65, 9)
    bad[7] = np.nan
    a, b = ch.project_batch([dict(points=bad, slot=0), dict(points=P, slot=2)])
    assert a["status"] == NOT_FINITE_STATUS and b["status"] == 0
    same(b, SLOTS[2], P, "beside a flagged item")


def test_inv_poly_lengths_missing_and_cleared(ch, lib, vio):
    cam = ref_cam(cr.SCARAMUZZA)
    P = points(65, 5)
    rng = np.random.RandomState(4)
    twenty = list(rng.uniform(-30.0, 30.0, 20) / (1.0 + np.arange(20)) ** 2)
    twenty[0] += 250.0
    for inv in ([263.5], twenty, twenty[:19]):
        ch.set_inv_poly(3, inv)
        out = ch.project_batch([dict(points=P, slot=3)])[0]
        same(out, cr.SCARAMUZZA, P, "%d coefficients" % len(inv), inv)
    a = cp.project(cam, P, twenty)[0]
    assert np.max(np.abs(a - cp.project(cam, P, twenty[:19])[0])) > 1e-9      # the twentieth enters
    # vio_camera_set on the slot clears it: the slot is refused, and nothing is written
    ch.set_camera(slot=3, **cr.SCARAMUZZA)
    pix, fl = np.full((65, 2), 7.5), np.full(65, 9, dtype=np.uint8)
    res = (C.c_int32 * 4)(5, 5, 5, 5)
    items = (ch_item(lib) * 2)()
    good = points(5, 1)
    gpix, gfl = np.full((5, 2), 7.5), np.full(5, 9, dtype=np.uint8)
    items[0] = ch_item(lib)(5, 0, good.ctypes.data, gpix.ctypes.data, gfl.ctypes.data)
    items[1] = ch_item(lib)(65, 3, P.ctypes.data, pix.ctypes.data, fl.ctypes.data)
    st = lib.fn["project_batch"](ch.h, C.c_int32(2), C.addressof(items), C.addressof(res))
    assert st == BAD_ARG and b"inv_poly" in lib.fn["last_error"](ch.h)
    assert np.all(pix == 7.5) and np.all(fl == 9) and np.all(gpix == 7.5) and np.all(gfl == 9) and list(res) == [5, 5, 5, 5]
    ch.set_inv_poly(3, inv_of(cr.SCARAMUZZA))
    same(ch.project_batch([dict(points=P, slot=3)])[0], cr.SCARAMUZZA, P, "set again")
    # a camera slot that was never SCARAMUZZA, coefficient counts out of range, values that are not finite
    for slot, inv in ((0, [1.0]), (3, []), (3, [1.0] * 21), (3, [1.0, np.nan]), (3, [np.inf]), (100, [1.0]), (-1, [1.0]), (256, [1.0])):
        with pytest.raises(vio.capi.VioError):
            ch.set_inv_poly(slot, inv)
    same(ch.project_batch([dict(points=P, slot=3)])[0], cr.SCARAMUZZA, P, "a refused set_inv_poly leaves the slot as it was")


def ch_item(lib):
    import conftest
    return conftest.load_package().camera.VioCameraProjectItem


def test_argument_errors_write_nothing(ch, lib):
    Item = ch_item(lib)
    P = points(5, 1)
    for n, slot, pts_null, pix_null, count in ((-1, 0, False, False, 1), (4097, 0, False, False, 1), (5, 9, False, False, 1), (5, 256, False, False, 1),
                                               (5, -1, False, False, 1), (5, 0, True, False, 1), (5, 0, False, True, 1), (5, 0, False, False, -1),
                                               (5, 0, False, False, 4097)):
        pix, fl = np.full((5, 2), 7.5), np.full(5, 9, dtype=np.uint8)
        items = (Item * 1)(Item(n, slot, None if pts_null else P.ctypes.data, None if pix_null else pix.ctypes.data, fl.ctypes.data))
        res = (C.c_int32 * 2)(5, 5)
        assert lib.fn["project_batch"](ch.h, C.c_int32(count), C.addressof(items), C.addressof(res)) == BAD_ARG, (n, slot, count)
        assert np.all(pix == 7.5) and np.all(fl == 9) and list(res) == [5, 5]
    res = (C.c_int32 * 2)(5, 5)
    assert lib.fn["project_batch"](ch.h, C.c_int32(0), None, None) == 0
    assert lib.fn["project_batch"](ch.h, C.c_int32(1), None, C.addressof(res)) == BAD_ARG
    # flags may be NULL
    pix = np.zeros((5, 2))
    items = (Item * 1)(Item(5, 0, P.ctypes.data, pix.ctypes.data, None))
    assert lib.fn["project_batch"](ch.h, C.c_int32(1), C.addressof(items), C.addressof(res)) == 0 and list(res) == [0, 0]
    assert pix.tobytes() == want(SLOTS[0], P)[0].tobytes()


def test_lift_is_what_it_was_before_and_after(ch):
    """vio_camera_lift_batch on the handle the new calls run on: the existing restatement's bytes, before and after them."""
    def lifts():
        outs = []
        for slot in (0, 2, 3, 6):                           # the models whose lift is exact in every bit
            cam = ref_cam(SLOTS[slot])
            c, r = cr.centre(cam), 0.9 * cr.field_radius(cam)
            px = (c + np.random.RandomState(slot).uniform(-1, 1, (130, 2)) * r / np.sqrt(2.0)).astype(np.float32)
            o = ch.lift_batch([dict(pts=px, slot=slot)])[0]
            ref = cam.lift(px)
            assert o["status"] == 0 and o["rays"].tobytes() == ref["rays"].tobytes(), slot
            outs.append(o["rays"].tobytes())
        return outs
    before = lifts()
    ch.project_batch([dict(points=points(257, s), slot=s) for s in SLOTS])
    ch.set_inv_poly(3, [250.0, 100.0])
    ch.project(points(65, 1), slot=3)
    assert lifts() == before
