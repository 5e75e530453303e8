"""libvio_aif_hip.so on the device against tests/aif_reference.py, bit for bit through vio_aif_frames_get: processIMU's and
processImage's parts at the sizes where the kernels change path (a wavefront of samples, a workgroup's chunk of points, the limits),
the refusals that must leave a slot as it was, slideWindow's erase, and the records of vio_aif_propagate_batch against
ImuHandle.load + propagate byte for byte; vio_aif_structure_batch against the restatement, ImuHandle and PnpHandle on synthetic
windows with non-keyframes at the front, in the middle and two in a row; initialize_from_frames against InitHandle.initialize_batch;
and StreamDriver(all_frames=) through run_batched."""
import numpy as np
import pytest

import aif_reference as ar
import aif_scenes as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(vio):
    return vio.load_aif()


@pytest.fixture()
def pair(lib):
    h = lib.create()
    yield h, ar.ImageFramesReference()
    h.close()


@pytest.fixture(scope="module")
def imu_handle(vio):
    h = vio.load_imu().create()
    yield h
    h.close()


def samples(rng, n):
    return rng.uniform(0.002, 0.006, n), rng.randn(n, 3) * 2 + [0, 0, 9.8], rng.randn(n, 3) * 0.3


def image(rng, n, lo=0, span=5000):
    ids = rng.choice(span, n, replace=False).astype(np.int64) + lo
    return ids, rng.uniform(-1, 1, (n, 2))


def both(pair, name, items):
    h, ref = pair
    got, want = getattr(h, name)(items), getattr(ref, name)(items)
    assert got == want, (name, got, want)
    return got


def check(pair, slots):
    h, ref = pair
    for s in slots:
        assert ar.same_slot(h.frames_get(s), ref.frames_get(s)), s


def fill(pair, rng, slot, frames, n_pts=7, n_smp=5, t0=10.0):
    """`frames` images on `slot`, each after n_smp samples (n_smp: an int or one per frame)."""
    counts = [n_smp] * frames if isinstance(n_smp, int) else list(n_smp)
    for j in range(frames):
        both(pair, "imu_batch", [(slot,) + samples(rng, counts[j])])
        ids, pts = image(rng, n_pts)
        both(pair, "image_batch", [(slot, t0 + 0.05 * j, ids, pts, rng.randn(3) * 0.01, rng.randn(3) * 0.001)])


def test_imu_runs_of_every_size_split_over_calls_and_before_the_first_image(pair):
    rng = np.random.RandomState(1)
    slots = [3, 0, 255, 17, 100]
    # before the first image the samples are dropped and acc_0 / gyr_0 follow
    both(pair, "imu_batch", [(s,) + samples(rng, n) for s, n in zip(slots, (0, 1, 63, 64, 65))])
    check(pair, slots)
    assert all(len(pair[0].frames_get(s)["open"]["dt"]) == 0 for s in slots)
    both(pair, "image_batch", [(s, 1.0) + image(rng, 5) + (np.zeros(3), np.zeros(3)) for s in slots])
    for counts in ((0, 1, 63, 64, 65), (65, 64, 63, 1, 0), (2, 2, 2, 2, 2)):
        both(pair, "imu_batch", [(s,) + samples(rng, n) for s, n in zip(slots, counts)])
        check(pair, slots)
    both(pair, "image_batch", [(s, 2.0) + image(rng, 3) + (rng.randn(3), rng.randn(3)) for s in slots])
    both(pair, "imu_batch", [(s,) + samples(rng, 4) for s in slots])
    check(pair, slots)
    assert [len(pair[0].frames_get(s)["frames"][1]["dt"]) for s in slots] == [67, 67, 128, 67, 67]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1024])
def test_image_points_are_stored_in_ascending_id(pair, n):
    rng = np.random.RandomState(n)
    ids, pts = image(rng, n, lo=-2000)                      # (negative ids too: the order is the signed one)
    ids[:n // 2] += 1 << 40                                 # ... and ids past 2^32
    both(pair, "imu_batch", [(9,) + samples(rng, 3)])
    both(pair, "image_batch", [(9, 0.5, ids, pts, np.zeros(3), np.zeros(3))])
    both(pair, "image_batch", [(9, 0.75) + image(rng, 6) + (np.ones(3), -np.ones(3))])
    check(pair, [9])
    got = pair[0].frames_get(9)["frames"][0]
    assert np.array_equal(got["ids"], np.sort(ids)) and np.array_equal(got["pts"], pts[np.argsort(ids)])


def test_argument_errors_leave_the_slot_as_it_was(vio, pair):
    rng = np.random.RandomState(2)
    h, ref = pair
    fill(pair, rng, 5, 3)
    ids, pts = image(rng, 8)
    bad = [(5, 20.0) + image(rng, 1025, span=9000) + (np.zeros(3), np.zeros(3)),                    # 1025 points
           (5, 20.0, np.concatenate([ids, ids[:1]]), np.concatenate([pts, pts[:1]]), np.zeros(3), np.zeros(3)),     # a duplicate id
           (5, 10.0 + 0.05 * 2, ids, pts, np.zeros(3), np.zeros(3)),                                # the last header again
           (5, 9.0, ids, pts, np.zeros(3), np.zeros(3))]                                            # an earlier one
    for item in bad:
        with pytest.raises(vio.VioError) as e:
            h.image_batch([item])
        assert e.value.status == -1
        with pytest.raises(ValueError):
            ref.image_batch([item])
        check(pair, [5])
    # a bad item refuses the whole call: the good item in front of it is not applied either
    with pytest.raises(vio.VioError):
        h.image_batch([(6, 1.0, ids, pts, np.zeros(3), np.zeros(3)), bad[2]])
    assert h.frames_get(6)["frames"] == []
    both(pair, "image_batch", [(5, 20.0, ids, pts, np.zeros(3), np.zeros(3))])
    check(pair, [5])


def test_frame_33_and_the_pools_refuse_with_the_slot_unchanged(pair):
    rng = np.random.RandomState(3)
    h, ref = pair
    fill(pair, rng, 7, 32, n_pts=3, n_smp=1)
    r = both(pair, "image_batch", [(7, 99.0) + image(rng, 3) + (np.zeros(3), np.zeros(3)), (8, 99.0) + image(rng, 3) + (np.zeros(3), np.zeros(3))])
    assert [x["status"] for x in r] == [ar.STATUS_FRAMES_FULL, ar.STATUS_OK] and r[0]["n_frames"] == 32
    check(pair, [7, 8])
    # the sample pool: 4096 fit, one more does not; the refused run moves neither the samples nor acc_0 / gyr_0
    both(pair, "imu_batch", [(8,) + samples(rng, 4000)])
    both(pair, "imu_batch", [(8,) + samples(rng, 96)])
    r = both(pair, "imu_batch", [(8,) + samples(rng, 1), (7,) + samples(rng, 1)])
    assert [x["status"] for x in r] == [ar.STATUS_POOL_FULL, ar.STATUS_OK] and r[0]["n_samples"] == 4096
    check(pair, [7, 8])
    # the point pool: 8 frames of 1024 fill it
    for j in range(8):
        both(pair, "image_batch", [(20, 1.0 + j) + image(rng, 1024 if j else 1021) + (np.zeros(3), np.zeros(3))])
    r = both(pair, "image_batch", [(20, 50.0) + image(rng, 4) + (np.zeros(3), np.zeros(3))])
    assert r[0]["status"] == ar.STATUS_POOL_FULL and r[0]["n_points"] == 8189
    r = both(pair, "image_batch", [(20, 50.0) + image(rng, 3) + (np.zeros(3), np.zeros(3))])
    assert r[0]["status"] == ar.STATUS_OK and r[0]["n_points"] == 8192
    check(pair, [20])


@pytest.mark.parametrize("case", ["first", "two_in_front", "last", "absent"])
def test_slide_erases_every_frame_up_to_t0(pair, case):
    rng = np.random.RandomState(4)
    fill(pair, rng, 30, 6, n_pts=300, n_smp=[0, 3, 70, 1, 0, 260])
    fill(pair, rng, 31, 4)
    both(pair, "imu_batch", [(30,) + samples(rng, 9)])      # the open interval holds samples and moves with the rest
    t = [f["t"] for f in pair[1].frames_get(30)["frames"]]
    t_0 = dict(first=t[0], two_in_front=t[2], last=t[-1], absent=0.5 * (t[1] + t[2]))[case]
    r = both(pair, "slide_batch", [(31, 10.0), (30, t_0)])
    assert r[1]["status"] == (ar.STATUS_NO_FRAME if case == "absent" else ar.STATUS_OK)
    assert r[1]["n_frames"] == dict(first=5, two_in_front=3, last=0, absent=6)[case] and r[0]["n_frames"] == 3
    check(pair, [30, 31])
    # the slot goes on as the restatement's does
    both(pair, "imu_batch", [(30,) + samples(rng, 5)])
    both(pair, "image_batch", [(30, 77.0) + image(rng, 11) + (rng.randn(3), rng.randn(3))])
    check(pair, [30])


@pytest.mark.parametrize("dropped", [0, 1, 1025])
def test_slide_drops_an_interval_of_any_size(pair, dropped):
    rng = np.random.RandomState(5)
    fill(pair, rng, 40, 5, n_pts=2, n_smp=[0, dropped, 600, 1030, 2])      # frames 0 and 1 leave: `dropped` samples; 1632 move down
    t = [f["t"] for f in pair[1].frames_get(40)["frames"]]
    r = both(pair, "slide_batch", [(40, t[1])])
    assert r[0]["erased_samples"] == dropped and r[0]["erased_frames"] == 2 and r[0]["n_samples"] == 1632
    check(pair, [40])


def test_reset_keeps_acc_0_and_clears_the_map(pair):
    rng = np.random.RandomState(6)
    h, ref = pair
    fill(pair, rng, 50, 3)
    h.reset(50)
    ref.reset(50)
    check(pair, [50])
    assert np.any(h.frames_get(50)["acc_0"] != 0)
    both(pair, "imu_batch", [(50,) + samples(rng, 4)])      # dropped again: no image since the reset
    both(pair, "image_batch", [(50, 1.0) + image(rng, 4) + (np.zeros(3), np.zeros(3))])      # (an earlier header is fine after a reset)
    check(pair, [50])


def records(out, n):
    return np.frombuffer(out, dtype=np.float64)[:467 * n].reshape(n, 467)


def test_propagate_equals_imu_handle_load_and_propagate_byte_for_byte(vio, pair, imu_handle):
    rng = np.random.RandomState(7)
    h, ref = pair
    fill(pair, rng, 60, 6, n_smp=[4, 0, 1, 63, 64, 65])     # interval 1 is empty: the empty record of vio_imu.h
    fill(pair, rng, 61, 2, n_smp=20)
    fill(pair, rng, 62, 1)
    slots, ba, bg = [61, 60, 62, 63], rng.randn(4, 3) * 0.05, rng.randn(4, 3) * 0.005
    res = vio.BatchImageFrames(h, slots).propagate(ba, bg)
    assert [r["records"] for r in res] == [1, 5, 0, 0]
    for i, s in enumerate(slots):
        ivs = ar.intervals(ref.frames_get(s))
        if not ivs:
            continue
        imu_handle.load(ivs)
        want = (vio.VioPreint * len(ivs))()
        imu_handle.propagate(ba[i], bg[i], out=want)
        assert records(res[i]["preint"], len(ivs)).tobytes() == records(want, len(ivs)).tobytes(), s
    empty = records(res[1]["preint"], 5)[0]
    assert empty[0] == 0 and np.array_equal(empty[4:8], [0, 0, 0, 1]) and np.array_equal(empty[11:17], np.concatenate([ba[1], bg[1]]))
    assert np.array_equal(empty[17:242].reshape(15, 15), np.eye(15)) and not empty[242:].any()
    again = vio.BatchImageFrames(h, slots[::-1]).propagate(ba[::-1], bg[::-1])
    for a, b in zip(res, again[::-1]):
        assert bytes(a["preint"]) == bytes(b["preint"])
    check(pair, slots)                                      # propagate changes nothing


def test_a_slot_does_not_depend_on_its_number_its_place_or_its_neighbours(lib):
    rng = np.random.RandomState(8)

    def script(seed, t_0):
        r = np.random.RandomState(seed)
        out = []
        for j in range(5):
            out.append(("imu_batch", samples(r, 30 + j + seed)))
            out.append(("image_batch", (1.0 + j,) + image(r, 100 + j + seed) + (r.randn(3), r.randn(3))))
        return out + [("slide_batch", (t_0,))]

    mine, left, right = script(0, 2.0), script(1, 3.0), script(2, 1.0)
    h = lib.create()
    for name, args in mine:                                 # alone on slot 0
        getattr(h, name)([(0,) + args])
    for (name, args), (_, la), (_, ra) in zip(mine, left, right):      # on slot 200, last in the batch, between two busy neighbours
        getattr(h, name)([(199,) + la, (201,) + ra, (200,) + args])
    a, b = h.frames_get(0), h.frames_get(200)
    assert len(a["frames"]) == 3 and ar.same_slot(a, b)
    assert ar.same_slot(h.frames_get(0), a)                 # a second download is the same
    h.close()


# ---- vio_aif_structure_batch ----
@pytest.fixture(scope="module")
def pnp_handle(vio):
    h = vio.load_pnp().create()
    yield h
    h.close()


def constructor_records(vio, imu_handle, slot_dict):
    """ImuHandle.load + propagate of the slot's intervals 1 .. F - 1, each at its constructor biases."""
    ivs = ar.intervals(slot_dict)
    bias = np.array([f["bias"] for f in slot_dict["frames"][1:]])
    imu_handle.load(ivs)
    want = (vio.VioPreint * len(ivs))()
    imu_handle.propagate(bias[:, 0:3], bias[:, 3:6], out=want)
    return records(want, len(ivs))


def expect(vio, imu_handle, pnp_handle, ref_slot, item, got):
    """Everything vio_aif_structure_batch returns for a slot, from the restatement, ImuHandle and PnpHandle."""
    F = len(ref_slot["frames"])
    rec = records(got["preint"], F - 1)
    assert rec.tobytes() == constructor_records(vio, imu_handle, ref_slot).tobytes()
    var = ar.excitation(rec)                                # the restatement's sums over the device's own records
    # var is bit for bit the restatement's where it is a number.  Where it is NaN (F = 1, or an interval without samples) this is
    # looser than "bit for bit": any NaN of the device is taken.  include/vio_aif.h leaves that NaN's sign and payload open, because
    # 0 / 0 sets the sign bit on an x86 host (the restatement here) and clears it on the device; the flag is held either way.
    assert (np.float64(got["var"]).tobytes() == np.float64(var).tobytes() or (np.isnan(var) and np.isnan(got["var"]))) and got["low_excitation"] == int(var < 0.25)
    st, is_key, guess = ar.walk([f["t"] for f in ref_slot["frames"]], item["headers"].tolist())
    assert got["status"] == st == ar.STATUS_OK and got["is_key"].tolist() == is_key and got["n_key"] == sum(is_key) and got["n_frames"] == F
    pitem = ar.pnp_item(ref_slot, item, is_key, guess)
    pnp = pnp_handle.frames_batch([pitem])[0]
    nk = [j for j in range(F) if not is_key[j]]
    assert got["pnp_status"] == pnp["status"] and got["fail_frame"] == (nk[pnp["fail_frame"]] if pnp["fail_frame"] >= 0 else -1)
    for name, key in (("frame_status", "frame_status"), ("iterations", "iterations"), ("n_used", "n_used"), ("cost", "cost")):
        assert got[name][nk].tobytes() == pnp[key].tobytes(), name
    assert got["T"][nk].tobytes() == pnp["T"].tobytes()     # T_pnp goes through unchanged; Q_pnp is held through R below
    R, T = ar.finish(ref_slot, item, is_key, guess, pnp)
    assert got["R"].reshape(F, 9).tobytes() == R.tobytes() and got["T"].tobytes() == T.tobytes()
    return is_key, guess, pnp, rec


@pytest.mark.parametrize("pattern", ["front", "middle", "full"])
def test_structure_equals_the_restatement_the_imu_and_the_pnp_library(vio, pair, imu_handle, pnp_handle, pattern):
    h, ref = pair
    scene = sc.make(pattern, seed=len(pattern))
    sc.feed(h, 11, scene)
    sc.feed(ref, 11, scene)
    got = h.structure_batch([dict(scene["item"], slot=11)])[0]
    is_key, guess, pnp, rec = expect(vio, imu_handle, pnp_handle, ref.frames_get(11), scene["item"], got)
    assert is_key == scene["is_key"] and pnp["status"] == 0 and np.all(pnp["frame_status"] == 0)      # no frame is left out
    check(pair, [11])                                       # R, T and is_key went into the slot as into the restatement's
    # ... and within 1e-14 of all_frames_to_init_items (its matmul is not order-pinned; entries at most 1, three products each)
    sfm = [dict(status=0, Q=scene["item"]["Q"], T=scene["item"]["T"])]
    init = vio.all_frames_to_init_items(sfm, [pnp], sc.RIC, [list(range(len(is_key) - 1))], [is_key])[0]
    assert np.abs(init["R"] - got["R"]).max() <= 1e-14 and np.abs(init["T"] - got["T"]).max() <= 1e-14
    # the poses are the scene's: the PnP found every non-keyframe
    for j in range(len(is_key)):
        q, p = sc.pose(j)
        assert np.abs(got["T"][j] - p).max() < 1e-6 and np.abs(got["R"][j] - np.array(ar.quat_to_rot(q)).reshape(3, 3) @ sc.RIC.T).max() < 1e-6
    again = h.structure_batch([dict(scene["item"], slot=11)])[0]
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in ("R", "T", "is_key", "cost", "iterations")) and bytes(got["preint"]) == bytes(again["preint"])


def test_structure_five_points_fail_a_frame_six_do_not_and_a_nan_point_fails_its_slot_only(vio, pair, imu_handle, pnp_handle):
    h, ref = pair
    base = sc.make("middle", seed=21)
    five, six = sc.thin(base, 2, 5), sc.thin(base, 2, 6)
    nan = dict(base, item=dict(base["item"], points=base["item"]["points"].copy()))
    live = np.nonzero(base["item"]["state"])[0]
    nan["item"]["points"][live[0], 1] = np.nan              # a NaN coordinate of a track with state 1
    scenes = {40: five, 41: six, 42: nan, 43: base}
    for s, scn in scenes.items():
        sc.feed(h, s, scn)
        sc.feed(ref, s, scn)
    got = h.structure_batch([dict(scn["item"], slot=s) for s, scn in scenes.items()])
    for g, (s, scn) in zip(got, scenes.items()):
        expect(vio, imu_handle, pnp_handle, ref.frames_get(s), scn["item"], g)
    assert got[0]["pnp_status"] == vio.pnp.FAIL_FEW_POINTS and got[0]["fail_frame"] == 2 and got[0]["n_used"][2] == 5
    assert np.isnan(got[0]["R"][2]).all() and got[0]["frame_status"][[6, 7, 12]].tolist() == [0, 0, 0] and np.isfinite(got[0]["R"][[6, 7, 12]]).all()
    assert got[1]["pnp_status"] == 0 and got[1]["n_used"][2] == 6
    assert got[2]["pnp_status"] == vio.pnp.NOT_FINITE and np.isnan(got[2]["R"][[2, 6, 7, 12]]).all() and np.isfinite(got[2]["R"][0]).all()
    assert got[3]["pnp_status"] == 0 and np.isfinite(got[3]["R"]).all()
    check(pair, list(scenes))
    # slot 43's bits do not depend on its neighbours, its place or its number
    sc.feed(h, 200, base)
    alone = h.structure_batch([dict(base["item"], slot=200)])[0]
    assert all(np.asarray(alone[k]).tobytes() == np.asarray(got[3][k]).tobytes() for k in ("R", "T", "is_key", "cost", "iterations", "n_used"))
    assert bytes(alone["preint"]) == bytes(got[3]["preint"]) and alone["var"] == got[3]["var"]


def test_structure_walk_failures_solve_nothing_and_leave_the_slot(pair):
    h, ref = pair
    scene = sc.make("front", seed=5)
    sc.feed(h, 3, scene)
    sc.feed(ref, 3, scene)
    before = h.frames_get(3)
    hd = scene["item"]["headers"]
    for headers in (np.concatenate([hd[:4], [hd[4] + 0.01], hd[5:]]),      # a header found in no frame
                    hd[:-1]):                                              # i runs past n_key at the last frame
        item = dict(scene["item"], slot=3, headers=headers, Q=scene["item"]["Q"][:len(headers)], T=scene["item"]["T"][:len(headers)])
        got = h.structure_batch([item])[0]
        assert ar.walk([f["t"] for f in before["frames"]], headers.tolist())[0] == ar.STATUS_WALK
        assert got["status"] == ar.STATUS_WALK and got["pnp_status"] == 0 and got["fail_frame"] == -1 and not got["is_key"].any()
        assert np.isnan(got["R"]).all() and np.isnan(got["T"]).all() and got["n_frames"] == 12
        assert ar.same_slot(h.frames_get(3), before)


def test_structure_refuses_a_non_finite_keyframe_pose_and_leaves_the_slot(vio, pair):
    h, ref = pair
    scene = sc.make("front", seed=5)
    sc.feed(h, 3, scene)
    before = h.frames_get(3)
    for name in ("Q", "T"):
        bad = scene["item"][name].copy()
        bad[10, 1] = np.nan                                 # the last keyframe: no non-keyframe takes it as its guess
        with pytest.raises(vio.VioError):
            h.structure_batch([dict(scene["item"], slot=3, **{name: bad})])
        assert ar.same_slot(h.frames_get(3), before)


def test_initialize_from_frames_equals_initialize_batch_on_the_same_records_and_items(vio, pair, imu_handle, pnp_handle):
    """The four calls against InitHandle.initialize_batch fed the library's own constructor records and the restatement's R / T."""
    h, ref = pair
    ih = vio.load_init().create()
    scenes = {7: sc.make("middle", seed=6), 90: sc.make("front", seed=5), 8: sc.thin(sc.make("middle", seed=21), 2, 5)}
    for s, scn in scenes.items():
        sc.feed(h, s, scn)
        sc.feed(ref, s, scn)
    sfm = [dict(status=0, Q=scn["item"]["Q"], T=scn["item"]["T"], points=scn["item"]["points"], state=scn["item"]["state"]) for scn in scenes.values()]
    sfm.append(dict(status=3))                              # a slot whose SfM failed: no try
    frames = vio.BatchImageFrames(h, list(scenes) + [9])
    tic, g_norm = sc.TIC, 9.81
    out = vio.initialize_from_frames(frames, ih, sfm, [scn["item"]["headers"] for scn in scenes.values()] + [None],
                                     [scn["item"]["track_ids"] for scn in scenes.values()] + [None], sc.RIC, tic, g_norm)
    assert out[2] is None and out[3] is None                # the PnP failed a frame; the SfM failed
    items, ivs = [], []
    for o, (s, scn) in zip(out[:2], scenes.items()):
        slot = ref.frames_get(s)
        st, is_key, guess = ar.walk([f["t"] for f in slot["frames"]], scn["item"]["headers"].tolist())
        pnp = pnp_handle.frames_batch([ar.pnp_item(slot, scn["item"], is_key, guess)])[0]
        R, T = ar.finish(slot, scn["item"], is_key, guess, pnp)
        F = len(is_key)
        items.append(dict(R=R.reshape(F, 3, 3), T=T, pre=[o["structure"]["preint"][j] for j in range(F - 1)], is_key=is_key))
        ivs.append(ar.intervals(slot))
    want = ih.initialize_batch(items, ivs, imu_handle, tic, g_norm)
    for o, w in zip(out[:2], want):
        # the scenes' samples are the path's own (tests/aif_scenes.py), so both windows, each with non-keyframes, are aligned: the bits
        # compared below are numbers, and they are the scene's scale, gravity and gyro bias
        assert o["status"] == w["status"] == 0 and o["n_key"] == w["n_key"] == 11 and not o["structure"]["is_key"].all()
        for k in ("s", "g", "g_world", "s_linear", "g_linear", "bg", "poses", "speed_bias", "x", "rot"):
            assert np.isfinite(o[k]).all() and np.isfinite(w[k]).all(), k
        assert o["poses"].shape == (11, 7) and o["speed_bias"].shape == (11, 9) and o["x"].shape == (3 * o["structure"]["n_frames"] + 3,)
        assert abs(o["s"] - sc.SCALE) < 0.05 * sc.SCALE and np.abs(o["g"] - sc.GRAVITY).max() < 0.1 and np.abs(o["bg"] - sc.BG_TRUE).max() < 0.005
        for k in ("s", "g", "g_world", "s_linear", "g_linear", "bg", "poses", "speed_bias", "x", "rot"):
            assert np.asarray(o[k]).tobytes() == np.asarray(w[k]).tobytes(), k
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(o["pre"], w["pre"]) for k in ("delta_p", "delta_q", "delta_v", "jacobian", "covariance"))
    ih.close()


DRIVER_DIFF_MEASURED = 3.3e-6     # m, the largest position difference on the first device run; the bound is ten times it


def test_stream_drivers_with_all_frames_run_like_the_drivers_without(vio, hip_lib, lib):
    """Three synthetic streams through run_batched with their tries taken from resident all_image_frame slots, against the same
    drivers without.  The two differ only in which pre-integration feeds the gyro step: the slot's records at the constructor biases
    against the driver's own records."""
    from vio_amd import batch_stream, stream as vs
    PX = 1.0 / 460.0
    make = lambda s: vs.SyntheticStream(n_frames=16, landmarks_per_frame=60, track_len=10, seed=s, pixel_noise=0.1 * PX)
    ah = lib.create()

    def run(with_frames):
        first = vs.StreamDriver(hip_lib, make(0), initialize=dict(sfm=True, all_frames=(ah, 5)) if with_frames else dict(sfm=True))
        sh = first.ctx.get_stream()
        ds = [first] + [vs.StreamDriver(hip_lib, make(s), ctx_kwargs=dict(stream=sh),
                                        initialize=dict(sfm=True, all_frames=(ah, 5 + 100 * s)) if with_frames else dict(sfm=True)) for s in (1, 2)]
        return ds, batch_stream.run_batched(ds, vio.load_marg().create(stream=sh))

    # an aligner cannot be combined with all_frames, and the stream's IMU noise must be the handle's: both are refused, not ignored
    with pytest.raises(ValueError, match="aligner"):
        vs.StreamDriver(hip_lib, make(0), initialize=dict(sfm=True, all_frames=(ah, 5), aligner=lambda *a: []))
    ah.set_config(noise=(0.1, 0.2121, 7.07e-6, 7.07e-7))
    with pytest.raises(ValueError, match="noise"):
        vs.StreamDriver(hip_lib, make(0), initialize=dict(sfm=True, all_frames=(ah, 5)))
    ah.set_config()
    da, ta = run(True)
    db, tb = run(False)
    diff = 0.0
    for a, b, x, y in zip(da, db, ta, tb):
        assert a.init_tries == b.init_tries and a.init_frame == b.init_frame and a.init_result["status"] == 0
        assert a.init_result["structure"]["n_frames"] == 11 and a.init_result["structure"]["is_key"].all()
        assert x.shape == y.shape
        diff = max(diff, float(np.abs(x[:, 1:4] - y[:, 1:4]).max()))
    print("largest position difference with / without all_frames: %.3e m" % diff)
    assert DRIVER_DIFF_MEASURED is not None and diff <= 10 * DRIVER_DIFF_MEASURED, diff
    ah.close()
