"""The forward-backward check of the batched Lucas-Kanade tracker on the GPU (include/vio_flow_back.h, k_flow_track<INV, true>) against
its numpy restatement (tests/flow_back_reference.py over tests/flow_reference.py, order "wave64"), on the fixture that reaches every
outcome.  next_pts, both statuses, back_pts, the iteration counts and d2 agree bit for bit; the costs under tests/test_gpu_flow.py's
rule for them (the NaNs in the same places, rtol = atol = 1e-9)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_reference as fb  # noqa: E402
import flow_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG = -1
L = fb.FIXTURE_LEVELS
EXACT = ("next_pts", "status", "iterations", "back_pts", "back_status", "back_iterations", "back_d2")
ALL = EXACT + ("cost", "back_cost")


@pytest.fixture(scope="module")
def flow_lib(vio, hip_lib):
    return vio.load_flow()


@pytest.fixture()
def fh(flow_lib):
    h = flow_lib.create()
    yield h
    h.close()


def same(got, ref, name, keys=ALL):
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (name, k, g.dtype, r.dtype, g.shape, r.shape)
        assert g.tobytes() == r.tobytes(), (name, k, "%d of %d entries differ" % (int(np.sum(g != r)), g.size))


def against_restatement(got, ref, name):
    c = fb.counts(ref)
    print("%s: %s; device kept %d" % (name, c, int(np.sum(got["status"] == fb.OK))))
    same(got, ref, name, EXACT)
    for k in ("cost", "back_cost"):
        g, r = got[k], ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.allclose(g[~np.isnan(g)], r[~np.isnan(r)], rtol=1e-9, atol=1e-9), (name, k)


def bytes_of(out):
    return b"".join(np.asarray(out[k]).tobytes() for k in ALL)


@pytest.mark.parametrize("inverse,back_levels", [(0, 2), (0, 0), (1, 2), (1, 0)])
def test_fixture_against_the_restatement(fh, inverse, back_levels):
    a, b, pts = fb.fixture()
    fh.set_config(levels=L, inverse=inverse)
    fh.set_back(levels=back_levels)
    got = fh.track(a, b, pts, back=True)
    ref = fb.fixture_reference(inverse, back_levels)
    c = fb.counts(ref)
    assert min(c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) >= 5, c
    against_restatement(got, ref, "fixture inv%d back levels %d" % (inverse, back_levels))
    # vio_flow_track_batch applies the check too: the same forward rows, no backward rows
    plain = fh.track(a, b, pts)
    assert sorted(plain) == ["cost", "iterations", "next_pts", "status"]
    same(plain, got, "track_batch with the check on", ("next_pts", "status", "iterations", "cost"))


@pytest.mark.parametrize("inverse", [0, 1])
def test_three_items_in_one_call(fh, inverse):
    a, b, pts = fb.fixture()
    sa, sb = fr.texture(33, 25, 8), fr.texture(33, 25, 8, shift=(0.6, -0.4))
    one = np.array([[16.2, 12.4]], dtype=np.float32)
    none = np.zeros((0, 2), dtype=np.float32)
    fh.set_config(levels=2, inverse=inverse)
    fh.set_back(levels=2)
    items = [dict(img_prev=a, img_next=b, prev_pts=pts), dict(img_prev=sa, img_next=sb, prev_pts=one), dict(img_prev=sb, img_next=sa, prev_pts=none)]
    outs = fh.track_batch(items, back=True)
    assert [len(o["status"]) for o in outs] == [140, 1, 0] and all(len(o["back_d2"]) == len(o["status"]) for o in outs)
    for i, it in enumerate(items):
        alone = fh.track_batch([it], back=True)[0]
        assert bytes_of(alone) == bytes_of(outs[i]), i
    again = fh.track_batch(items, back=True)
    assert [bytes_of(o) for o in again] == [bytes_of(o) for o in outs]
    ref = fb.track_back(sa, sb, one, levels=2, back_levels=2, inverse=inverse)
    against_restatement(outs[1], ref, "33 x 25, one point, inv%d" % inverse)
    assert outs[1]["back_status"][0] != fb.BACK_NOT_RUN


@pytest.mark.parametrize("inverse", [0, 1])
def test_forward_statuses_pass_through(fh, inverse):
    a, b, pts = fb.fixture()
    ref = fb.fixture_reference(inverse, 2)
    lost = int(np.nonzero(ref["status"] == fb.FAIL_LOST)[0][0])
    fh.set_config(levels=L, inverse=inverse)
    fh.set_back(levels=2)
    base = fh.track(a, b, pts, back=True)
    # a NaN keypoint in front, and the lost one among the rest
    more = np.concatenate([np.array([[np.nan, 10.0]], dtype=np.float32), pts])
    got = fh.track(a, b, more, back=True)
    assert got["status"][0] == fb.NOT_FINITE and got["status"][1 + lost] == fb.FAIL_LOST
    for k in (0, 1 + lost):
        assert got["back_status"][k] == fb.BACK_NOT_RUN and got["back_iterations"][k] == 0
        assert np.all(np.isnan(got["back_pts"][k])) and np.isnan(got["back_cost"][k]) and np.isnan(got["back_d2"][k])
    assert np.all(np.isnan(got["next_pts"][0]))
    same({k: got[k][1:] for k in ALL}, base, "the rows behind the NaN keypoint")
    # without the lost keypoint the others are what they were
    keep = np.arange(len(pts)) != lost
    fewer = fh.track(a, b, pts[keep], back=True)
    same(fewer, {k: base[k][keep] for k in ALL}, "the rows without the lost keypoint")


@pytest.mark.parametrize("inverse", [0, 1])
def test_forward_border_failure_stays(fh, inverse):
    a, b, pts = fb.fixture()
    cfg = dict(levels=L, inverse=inverse, border=20)
    fh.set_config(**cfg)
    fh.set_back(levels=2)
    got = fh.track(a, b, pts, back=True)
    ref = fb.track_back(a, b, pts, levels=L, back_levels=2, inverse=inverse, border=20)
    out = ref["status"] == fb.FAIL_BORDER
    assert out.sum() >= 5 and np.sum(ref["back_status"] != fb.BACK_NOT_RUN) >= 5
    against_restatement(got, ref, "border 20 inv%d" % inverse)
    assert np.all(got["status"][out] == fb.FAIL_BORDER) and np.all(got["back_status"][out] == fb.BACK_NOT_RUN)
    assert np.all(np.isfinite(got["next_pts"][out])) and np.all(np.isnan(got["back_d2"][out]))


@pytest.mark.parametrize("inverse", [0, 1])
def test_boundary_values_of_max_dist(fh, inverse):
    a, b, pts = fb.fixture()
    fh.set_config(levels=L, inverse=inverse)
    fh.set_back(levels=2)
    base = fh.track(a, b, pts, back=True)
    ran, came_back = base["back_status"] != fb.BACK_NOT_RUN, base["back_status"] == fb.OK
    fh.set_back(levels=2, max_dist=0.0)
    zero = fh.track(a, b, pts, back=True)
    exact = came_back & np.all(zero["back_pts"] == pts, axis=1)
    assert np.array_equal(zero["status"] == fb.OK, exact) and np.array_equal(zero["back_d2"][ran] == 0.0, exact[ran])
    assert np.all(zero["status"][came_back & ~exact] == fb.FAIL_BACK_FAR)
    fh.set_back(levels=2, max_dist=1e30)
    wide = fh.track(a, b, pts, back=True)
    assert np.array_equal(wide["status"] == fb.OK, came_back) and not np.any(wide["status"] == fb.FAIL_BACK_FAR)
    assert np.all(wide["status"][ran & ~came_back] == fb.FAIL_BACK_LOST)
    # max_dist enters the verdict alone
    for o in (zero, wide):
        same(o, base, "max_dist", tuple(k for k in ALL if k != "status"))


@pytest.mark.parametrize("inverse", [0, 1])
def test_check_off_is_the_tracker_as_it_was(flow_lib, vio, inverse):
    a, b, pts = fb.fixture()
    guess = (pts + np.array([0.5, -0.25], dtype=np.float32)).astype(np.float32)
    never, toggled = flow_lib.create(), flow_lib.create()
    try:
        for h in (never, toggled):
            h.set_config(levels=L, inverse=inverse)
        before = [toggled.track(a, b, pts), toggled.track(a, b, pts, guess)]
        toggled.set_back(levels=2)
        on = toggled.track(a, b, pts)
        assert np.any(on["status"] >= fb.FAIL_BACK_LOST)
        toggled.set_back(enabled=False)
        for h in (never, toggled):
            after = [h.track(a, b, pts), h.track(a, b, pts, guess)]
            for x, y in zip(before, after):
                assert sorted(y) == ["cost", "iterations", "next_pts", "status"]
                same(y, x, "check off", ("next_pts", "status", "iterations", "cost"))
        # ... which is the restatement's forward pass
        ref = fr.multi_level(a, b, pts, levels=L, inverse=inverse, order="wave64")
        assert np.array_equal(before[0]["status"], ref[1]) and before[0]["next_pts"].tobytes() == ref[0].tobytes()
        with pytest.raises(vio.VioError) as e:
            never.track(a, b, pts, back=True)                       # the check is off
        assert e.value.status == BAD_ARG, e.value
    finally:
        never.close()
        toggled.close()


def test_argument_rules(fh, vio):
    a, b, pts = fb.fixture()
    fh.set_config(levels=2)

    def refused(call):
        with pytest.raises(vio.VioError) as e:
            call()
        assert e.value.status == BAD_ARG, e.value

    refused(lambda: fh.set_back(levels=3))
    refused(lambda: fh.set_back(max_dist=-1.0))
    refused(lambda: fh.set_back(max_dist=float("nan")))
    refused(lambda: fh.track(a, b, pts, back=True))                 # still off: nothing was taken
    fh.set_back(levels=2)
    refused(lambda: fh.set_config(levels=1))                        # below the check's levels
    got = fh.track(a, b, pts, back=True)                            # the handle is as it was: 2 levels, the check over 2
    same(got, fb.track_back(a, b, pts, levels=2, back_levels=2), "after the refused calls", EXACT)


def test_resident_twin(vio, hip_lib, fh):
    a, b, pts = fb.fixture()
    fr_h = vio.load_frame().create()
    try:
        for inverse in (0, 1):
            fh.set_config(levels=L, inverse=inverse)
            fh.set_back(levels=2)
            fr_h.set_config(equalize=False, flow=dict(levels=L, inverse=inverse))
            fr_h.set_flow_back(levels=2)
            fr_h.push(a, slot=3)
            fr_h.push(b, slot=3)
            got, ref = fr_h.track(pts, slot=3, back=True), fh.track(a, b, pts, back=True)
            assert np.any(ref["status"] == fb.FAIL_BACK_FAR) and np.any(ref["status"] == fb.OK)
            same(got, ref, "resident inv%d" % inverse)
            same(fr_h.track(pts, slot=3), ref, "resident track_batch with the check on", ("next_pts", "status", "iterations", "cost"))
            fr_h.set_flow_back(enabled=False)
            with pytest.raises(vio.VioError) as e:
                fr_h.track(pts, slot=3, back=True)
            assert e.value.status == BAD_ARG
            fr_h.reset(3)
    finally:
        fr_h.close()
