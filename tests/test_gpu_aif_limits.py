"""vio_aif_structure_batch (include/vio_aif.h) where tests/test_gpu_aif.py does not take it: track tables of more
than one pass of k_aif_join's 256 threads (up to the 4096 the LDS table holds), frames of more observations than a wavefront and a
workgroup with the unusable ones at the positions where a strided copy or a prefix count breaks, a full point pool beside small
neighbours, the window shapes at the edges (F = 0, 1, 2, 32 keyframes, an interval without samples, a body at rest, another
min_points), tries, slides and resets in sequence on one slot, initialize_from_frames with every outcome in one batch, and the
argument rules of the header.

The rule is test_gpu_aif.py's expect(): records byte for byte ImuHandle's, var bit for bit the restatement's sums over them (where
those are NaN, any NaN: expect() says why), the walk the restatement's, the PnP's rows byte for byte PnpHandle.frames_batch's on the restatement's item, R / T bit for bit the restatement's
products, the slot afterwards the restatement's.  Every solved frame of 64 observations or more is also held to two references that
share no kernel text with the join or the PnP (independent()): n_used against a count in plain numpy over the ids, and T, cost and R
against tests/pnp_reference.py's frames(order="wave64") under test_gpu_pnp.py's rule (10 x the restatement's spread under two one-ulp
perturbations plus 1e-13 of the quantity's size).  tests/test_aif_reference.py checks on the CPU that the scenes (aif_scenes.LIMIT_SCENES)
do what is relied on here: which frames solve and which fail, with which n_used, that none is undecidable, and that var is far from 0.25.

Printed with -s: per solved frame of 64 observations or more its error and bar in T, cost and R, and per test the number of such
frames."""
import ctypes as C

import numpy as np
import pytest

import aif_reference as ar
import aif_scenes as sc
import pnp_reference as pr
from test_gpu_aif import both, check, expect, imu_handle, lib, pair, pnp_handle, records  # noqa: F401  (four of them are fixtures)

pytestmark = pytest.mark.gpu
FEW = pr.FAIL_FEW_POINTS
RESULT_KEYS = ("status", "pnp_status", "fail_frame", "n_frames", "n_key", "low_excitation")


def out_bytes(g):
    """Every output of a structure item as bytes: R, T, is_key, the frame rows, the records, var and the result struct."""
    rows = [np.asarray(g[k]).tobytes() for k in ("R", "T", "is_key", "frame_status", "iterations", "n_used", "cost")]
    return rows + [records(g["preint"], max(g["n_frames"] - 1, 0)).tobytes(), np.float64(g["var"]).tobytes(), tuple(g[k] for k in RESULT_KEYS)]


def independent(ref_slot, item, got, name):
    """The solved frames of 64 observations or more against plain numpy and pnp_reference.frames; returns how many there were."""
    st, is_key, guess = ar.walk([f["t"] for f in ref_slot["frames"]], item["headers"].tolist())
    pitem = ar.pnp_item(ref_slot, item, is_key, guess)
    ref = pr.frames(pitem, order="wave64")
    rng = np.random.RandomState(5)
    runs = [pr.frames(pr.perturb_ulp(pitem, rng), order="wave64") for _ in range(2)]
    live = np.asarray(item["track_ids"])[np.asarray(item["state"]) != 0]
    rot = lambda q: np.array(ar.mul_rict(ar.quat_to_rot(q), item["ric"]))
    count = 0
    for m, j in enumerate([j for j in range(len(is_key)) if not is_key[j]]):
        ids = ref_slot["frames"][j]["ids"]
        if len(ids) < 64 or ref["frame_status"][m] != pr.OK:
            continue
        count += 1
        assert got["n_used"][j] == int(np.isin(ids, live).sum()), (name, j)
        assert all(r["iterations"][m] == ref["iterations"][m] for r in runs), (name, j, "undecidable: tests/test_aif_reference.py holds the cap of 0")
        assert got["frame_status"][j] == pr.OK and got["iterations"][j] == ref["iterations"][m], (name, j, got["iterations"][j], ref["iterations"][m])
        for key, g, w, ws in (("T", got["T"][j], ref["T"][m], [r["T"][m] for r in runs]), ("cost", got["cost"][j], ref["cost"][m], [r["cost"][m] for r in runs]),
                              ("R", got["R"][j].reshape(-1), rot(ref["Q"][m]), [rot(r["Q"][m]) for r in runs])):
            sp = max(float(np.max(np.abs(x - w))) for x in ws)
            bar = 10.0 * sp + 1e-13 * max(1.0, float(np.max(np.abs(w))))
            err = float(np.max(np.abs(g - w)))
            print("%-12s frame %2d %-4s err %.3e  bar %.3e  obs %4d  n %4d  it %d" % (name, j, key, err, bar, len(ids), got["n_used"][j], got["iterations"][j]))
            assert err <= bar, (name, j, key, err, bar)
    print("%-12s frames of 64 observations or more held to numpy and pnp_reference.frames: %d" % (name, count))
    return count


def run(vio, pair, imu_handle, pnp_handle, slot, scene, item=None, feed=True):
    """The scene into `slot` of both, one structure call, expect() and the slot afterwards."""
    h, ref = pair
    item = scene["item"] if item is None else item
    if feed:
        sc.feed(h, slot, scene)
        sc.feed(ref, slot, scene)
    got = h.structure_batch([dict(item, slot=slot)])[0]
    is_key, guess, pnp, rec = expect(vio, imu_handle, pnp_handle, ref.frames_get(slot), item, got)
    check(pair, [slot])
    return got, pnp


# ---- a. the track table ----
@pytest.mark.parametrize("n_tracks", [0, 1, 255, 256, 257, 4096])
def test_track_tables_below_at_and_above_one_pass_of_the_join(vio, pair, imu_handle, pnp_handle, n_tracks):
    scene = sc.limit_scene("tracks%d" % n_tracks)
    got, pnp = run(vio, pair, imu_handle, pnp_handle, 17, scene)
    item = scene["item"]
    assert got["is_key"].tolist() == [0, 1, 1] and np.isfinite(got["R"][1:]).all() and np.array_equal(got["T"][1:], item["T"])      # the keyframes' rows are written
    if n_tracks <= 1:                                       # n_tracks 0: the extra invalid row is row 0
        assert (got["pnp_status"], got["fail_frame"], got["frame_status"][0], got["n_used"][0]) == (FEW, 0, FEW, n_tracks)
        assert np.isnan(got["R"][0]).all() and np.isnan(got["T"][0]).all() and np.isnan(got["cost"][0])
        return
    assert got["pnp_status"] == 0 and got["fail_frame"] == -1 and np.isfinite(got["R"]).all()
    assert got["n_used"][0] == dict([(255, 251), (256, 252), (257, 253), (4096, 1017)])[n_tracks]
    assert independent(pair[1].frames_get(17), item, got, "tracks%d" % n_tracks) == 1
    q, p = sc.pose(0)                                       # ... and the pose is the scene's
    assert np.abs(got["T"][0] - p).max() < 1e-6 and np.abs(got["R"][0] - np.array(ar.quat_to_rot(q)).reshape(3, 3) @ sc.RIC.T).max() < 1e-6
    if n_tracks == 4096:                                    # the dead tracks at sorted positions 0, 255, 256 and 4095 are observed, and dropped
        dead = item["track_ids"][item["state"] == 0]
        assert np.array_equal(np.sort(dead), np.sort(item["track_ids"])[[0, 255, 256, 4095]]) and np.isin(dead, scene["frames"][0]["ids"]).all()
        assert len(scene["frames"][0]["ids"]) - got["n_used"][0] == 4 + 3


# ---- b. observations per non-keyframe ----
def test_non_keyframes_of_0_to_1024_observations_with_the_unusable_ones_at_the_chunk_edges(vio, pair, imu_handle, pnp_handle):
    scene = sc.limit_scene("sizes")
    got, pnp = run(vio, pair, imu_handle, pnp_handle, 5, scene)
    nk = [2 * k + 1 for k in range(10)]
    assert [len(f["ids"]) for f in pair[1].frames_get(5)["frames"]][1::2] == list(sc.SIZES)
    assert got["n_used"][nk].tolist() == [0, 5, 6, 61, 62, 62, 251, 252, 252, 1018]
    assert got["frame_status"][nk].tolist() == [FEW, FEW] + [0] * 8 and (got["pnp_status"], got["fail_frame"]) == (FEW, 1)      # five usable points fail, six solve
    assert np.isnan(got["R"][[1, 3]]).all() and np.isfinite(np.delete(got["R"], [1, 3], axis=0)).all() and np.isfinite(np.delete(got["T"], [1, 3], axis=0)).all()
    assert independent(pair[1].frames_get(5), scene["item"], got, "sizes") == 6
    for j in nk[2:]:
        q, p = sc.pose(j)
        assert np.abs(got["T"][j] - p).max() < 1e-6 and np.abs(got["R"][j] - np.array(ar.quat_to_rot(q)).reshape(3, 3) @ sc.RIC.T).max() < 1e-6


def test_a_frame_of_1024_observations_of_which_five_or_six_are_usable(vio, pair, imu_handle, pnp_handle):
    scene = sc.limit_scene("five_six_of_1024")
    got, pnp = run(vio, pair, imu_handle, pnp_handle, 6, scene)
    assert got["n_used"].tolist() == [0, 5, 6, 0] and got["frame_status"].tolist() == [0, FEW, 0, 0] and (got["pnp_status"], got["fail_frame"]) == (FEW, 1)
    assert np.isnan(got["R"][1]).all() and np.isfinite(got["R"][[0, 2, 3]]).all()
    assert independent(pair[1].frames_get(6), scene["item"], got, "6 of 1024") == 1


# ---- c. a full pool, unequal neighbours ----
def test_three_unequal_items_the_last_with_a_full_pool_in_any_order_place_and_handle(vio, lib, pair, imu_handle, pnp_handle):
    h, ref = pair
    scenes = [sc.make("front", seed=5), sc.limit_scene("nkk257"), sc.limit_scene("pool")]
    slots = [3, 250, 9]
    for s, scn in zip(slots, scenes):
        sc.feed(h, s, scn)
        sc.feed(ref, s, scn)
    assert [ar.n_points(ref.frames_get(s)) for s in slots][1:] == [95, 8192] and [len(scn["item"]["track_ids"]) for scn in scenes] == [40, 257, 4096]
    items = [dict(scn["item"], slot=s) for s, scn in zip(slots, scenes)]
    got = h.structure_batch(items)
    for g, s, scn in zip(got, slots, scenes):
        expect(vio, imu_handle, pnp_handle, ref.frames_get(s), scn["item"], g)
        assert g["pnp_status"] == 0 and np.isfinite(g["R"]).all()
    check(pair, slots)
    assert independent(ref.frames_get(250), scenes[1]["item"], got[1], "nkk257") == 1
    assert independent(ref.frames_get(9), scenes[2]["item"], got[2], "pool") == 8
    want = [out_bytes(g) for g in got]
    assert [out_bytes(g) for g in h.structure_batch(items[::-1])] == want[::-1]
    assert [out_bytes(h.structure_batch([it])[0]) for it in items] == want
    other = lib.create()                                    # another handle, other slot numbers, another order
    try:
        moved = [255, 0, 128]
        for s, scn in zip(moved, scenes):
            sc.feed(other, s, scn)
        order = [2, 0, 1]
        out = other.structure_batch([dict(scenes[k]["item"], slot=moved[k]) for k in order])
        assert [out_bytes(g) for g in out] == [want[k] for k in order]
    finally:
        other.close()


# ---- d. window shapes ----
def raw_call(lib, h, items, count=None, null=None):
    """vio_aif_structure_batch through the raw entry point with pattern-filled out arrays and results.  An item dict may carry n_key /
    n_tracks to say something else than its arrays' lengths; null: {item index: fields set to NULL}.  Returns the status and whether
    every out array and result is as it was."""
    from vio_amd import aif
    from vio_amd.capi import VioPreint
    from vio_amd.pnp import VioPnpFrameInfo
    n = max(len(items), count or 0, 1)
    arr, keep, outs = (aif.VioAifStructureItem * n)(), [], []
    for i, it in enumerate(items):
        hd, Q, T = (np.ascontiguousarray(it[k], dtype=np.float64).reshape(-1) for k in ("headers", "Q", "T"))
        ids, pts = np.ascontiguousarray(it["track_ids"], dtype=np.int64).reshape(-1), np.ascontiguousarray(it["points"], dtype=np.float64).reshape(-1)
        state = np.ascontiguousarray(np.asarray(it["state"]) != 0, dtype=np.uint8).reshape(-1)
        ric = np.ascontiguousarray(it["ric"], dtype=np.float64).reshape(-1)
        o = dict(R=np.full((32, 9), 7.5), T=np.full((32, 3), 7.5), is_key=np.full(32, 77, dtype=np.uint8), pre=(VioPreint * 31)(), info=(VioPnpFrameInfo * 32)())
        C.memset(C.addressof(o["pre"]), 0x55, C.sizeof(o["pre"]))
        C.memset(C.addressof(o["info"]), 0x55, C.sizeof(o["info"]))
        keep += [hd, Q, T, ids, pts, state]
        outs.append(o)
        arr[i] = aif.VioAifStructureItem(int(it["slot"]), int(it.get("n_key", len(hd))), int(it.get("n_tracks", len(ids))), 0, hd.ctypes.data, Q.ctypes.data, T.ctypes.data,
                                         ids.ctypes.data, pts.ctypes.data, state.ctypes.data, (C.c_double * 9)(*ric), o["R"].ctypes.data, o["T"].ctypes.data,
                                         o["is_key"].ctypes.data, C.addressof(o["pre"]), C.addressof(o["info"]))
        for f in (null or {}).get(i, ()):
            setattr(arr[i], f, None)
    for i in range(len(items), n):                          # (count beyond the items: copies, so that nothing read is out of bounds)
        arr[i] = arr[0]
    res = (aif.VioAifStructureResult * n)()
    C.memset(C.addressof(res), 0x55, C.sizeof(res))
    st = lib.fn["structure_batch"](h.h, C.c_int32(len(items) if count is None else count), C.addressof(arr), C.addressof(res))
    untouched = bytes(res) == b"\x55" * C.sizeof(res) and all(
        np.all(o["R"] == 7.5) and np.all(o["T"] == 7.5) and np.all(o["is_key"] == 77) and bytes(o["pre"]) == b"\x55" * C.sizeof(o["pre"]) and
        bytes(o["info"]) == b"\x55" * C.sizeof(o["info"]) for o in outs)
    return st, untouched, res, outs


def test_an_empty_slot_is_a_failed_walk_and_nothing_is_written(lib, pair):
    h, ref = pair
    item = dict(sc.limit_scene("one")["item"], slot=77)
    before = h.frames_get(77)
    assert ar.walk([], item["headers"].tolist()) == (ar.STATUS_WALK, None, None)
    got = h.structure_batch([item])[0]
    assert [got[k] for k in RESULT_KEYS] == [ar.STATUS_WALK, 0, -1, 0, 0, 0] and np.isnan(got["var"])
    assert got["R"].shape == (0, 3, 3) and got["T"].shape == (0, 3) and len(got["is_key"]) == 0 and len(got["cost"]) == 0
    st, untouched, res, outs = raw_call(lib, h, [item])
    assert st == 0 and [getattr(res[0], k) for k in RESULT_KEYS] == [ar.STATUS_WALK, 0, -1, 0, 0, 0] and np.isnan(res[0].var)
    assert all(np.all(o["R"] == 7.5) and np.all(o["T"] == 7.5) and np.all(o["is_key"] == 77) and bytes(o["pre"]) == b"\x55" * C.sizeof(o["pre"]) and
               bytes(o["info"]) == b"\x55" * C.sizeof(o["info"]) for o in outs)
    assert ar.same_slot(h.frames_get(77), before) and ar.same_slot(before, ar.new_slot())
    # ... also beside an item that solves: the empty one takes no record and no row of its neighbour's
    scene = sc.make("front", seed=5)
    sc.feed(h, 78, scene)
    alone = h.structure_batch([dict(scene["item"], slot=78)])[0]
    pairs = h.structure_batch([item, dict(scene["item"], slot=78)])
    assert [pairs[0][k] for k in RESULT_KEYS] == [ar.STATUS_WALK, 0, -1, 0, 0, 0] and out_bytes(pairs[1]) == out_bytes(alone)


def test_one_keyframe_alone_has_no_record_and_its_pose_is_the_sfm_s(pair):
    h, ref = pair
    scene = sc.limit_scene("one")
    sc.feed(h, 12, scene)
    sc.feed(ref, 12, scene)
    item = scene["item"]
    got = h.structure_batch([dict(item, slot=12)])[0]
    assert ar.walk([scene["frames"][0]["t"]], item["headers"].tolist()) == (ar.STATUS_OK, [1], [0])
    assert [got[k] for k in RESULT_KEYS] == [0, 0, -1, 1, 1, 0] and np.isnan(got["var"]) and np.isnan(ar.excitation(np.zeros((0, 467))))
    R, T = ar.finish(ref.frames_get(12), item, [1], [0], dict(status=0, frame_status=[], Q=[], T=[]))
    assert got["R"].reshape(1, 9).tobytes() == R.tobytes() and got["T"].tobytes() == T.tobytes() and got["is_key"].tolist() == [1]
    assert (got["frame_status"][0], got["iterations"][0], got["n_used"][0], got["cost"][0]) == (0, 0, 0, 0.0)
    check(pair, [12])


def test_two_frames_and_thirty_two_keyframes(vio, pair, imu_handle, pnp_handle):
    got, pnp = run(vio, pair, imu_handle, pnp_handle, 13, sc.limit_scene("two"))
    assert [got[k] for k in RESULT_KEYS] == [0, 0, -1, 2, 1, 1] and got["var"] == 0.0 and got["is_key"].tolist() == [0, 1]      # one record is its own average
    assert got["frame_status"][0] == 0 and got["n_used"][0] >= 6 and np.isfinite(got["R"]).all()
    got, pnp = run(vio, pair, imu_handle, pnp_handle, 14, sc.limit_scene("all_key"))
    assert [got[k] for k in RESULT_KEYS][:5] == [0, 0, -1, 32, 32] and got["is_key"].tolist() == [1] * 32 and len(pnp["Q"]) == 0
    assert not got["frame_status"].any() and not got["iterations"].any() and not got["n_used"].any() and got["cost"].tobytes() == np.zeros(32).tobytes()
    assert np.array_equal(got["T"], sc.limit_scene("all_key")["item"]["T"]) and np.isfinite(got["R"]).all()


def test_an_interval_without_samples_is_the_empty_record_and_moves_nothing_else(vio, pair, imu_handle, pnp_handle):
    gap, pnp_gap = run(vio, pair, imu_handle, pnp_handle, 15, sc.limit_scene("gap"))
    full, pnp_full = run(vio, pair, imu_handle, pnp_handle, 16, sc.limit_scene("no_gap"))
    rec = records(gap["preint"], 11)
    bias = pair[1].frames_get(15)["frames"][5]["bias"]
    assert rec[4, 0] == 0 and np.array_equal(rec[4, 4:8], [0, 0, 0, 1]) and np.array_equal(rec[4, 11:17], bias)       # vio_imu.h's empty record
    assert np.array_equal(rec[4, 17:242].reshape(15, 15), np.eye(15)) and not rec[4, 242:].any()
    assert np.isnan(gap["var"]) and gap["low_excitation"] == 0 and np.isfinite(full["var"]) and full["low_excitation"] == 0
    for k in ("R", "T", "is_key", "frame_status", "iterations", "n_used", "cost"):
        assert np.asarray(gap[k]).tobytes() == np.asarray(full[k]).tobytes(), k
    assert [gap[k] for k in RESULT_KEYS[:5]] == [full[k] for k in RESULT_KEYS[:5]] == [0, 0, -1, 12, 11]
    other = np.delete(np.arange(11), [4, 5])                # (the interval behind the gap starts from another acc_0 / gyr_0: the last sample there is)
    assert rec[other].tobytes() == records(full["preint"], 11)[other].tobytes()


def test_a_body_at_rest_sets_low_excitation_and_a_moving_one_does_not(vio, pair, imu_handle, pnp_handle):
    rest, _ = run(vio, pair, imu_handle, pnp_handle, 18, sc.limit_scene("rest"))
    moving, _ = run(vio, pair, imu_handle, pnp_handle, 19, sc.limit_scene("no_gap"))
    print("var at rest %.3e, moving %.3e" % (rest["var"], moving["var"]))
    assert rest["low_excitation"] == 1 and 0 <= rest["var"] < 1e-9 and moving["low_excitation"] == 0 and moving["var"] > 1.0
    assert rest["pnp_status"] == 0 and np.isfinite(rest["R"]).all()       # the flag fails nothing


def test_min_points_of_twenty_fails_nineteen_usable_points_and_solves_twenty(vio, lib, imu_handle):
    h, ph, ref = lib.create(), vio.load_pnp().create(), ar.ImageFramesReference()
    scene = sc.limit_scene("nineteen_twenty")
    try:
        at_default, _ = run(vio, (h, ref), imu_handle, ph, 2, scene)
        assert at_default["frame_status"].tolist() == [0, 0, 0, 0] and at_default["n_used"].tolist() == [0, 19, 20, 0]
        h.set_config(min_points=20)
        ph.set_config(min_points=20)
        got, _ = run(vio, (h, ref), imu_handle, ph, 2, scene, feed=False)
        assert got["frame_status"].tolist() == [0, FEW, 0, 0] and got["n_used"].tolist() == [0, 19, 20, 0] and (got["pnp_status"], got["fail_frame"]) == (FEW, 1)
        assert np.isnan(got["R"][1]).all() and got["R"][2].tobytes() == at_default["R"][2].tobytes()
    finally:
        h.set_config()
        ph.set_config()
        h.close()
        ph.close()


# ---- e. sequences on one slot ----
def test_try_slide_three_new_images_try_again_equals_a_fresh_slot(vio, pair, imu_handle, pnp_handle):
    h, ref = pair
    scene = sc.limit_scene("longer")                        # the 15 frames of "middle" and three more: k, n, k
    first, tail, slid = sc.part(scene, 0, 15), sc.part(scene, 15, 18), sc.part(scene, 3, 18)
    got, _ = run(vio, pair, imu_handle, pnp_handle, 21, first)
    assert got["pnp_status"] == 0 and got["is_key"].tolist() == first["is_key"]
    r = both(pair, "slide_batch", [(21, first["frames"][2]["t"])])
    assert r[0]["status"] == ar.STATUS_OK and r[0]["n_frames"] == 12 and r[0]["erased_frames"] == 3
    check(pair, [21])
    left = h.frames_get(21)["frames"]                       # the rows that moved are not zeros
    assert [f["is_key"] for f in left] == first["is_key"][3:] and {0, 1} == set(first["is_key"][3:])
    assert all(np.isfinite(f["R"]).all() and np.abs(f["R"]).max() > 0.5 and np.any(f["T"] != 0) for f in left)
    assert np.array_equal(np.array([f["R"] for f in left]), got["R"][3:].reshape(12, 9)) and np.array_equal(np.array([f["T"] for f in left]), got["T"][3:])
    sc.feed(h, 21, tail)
    sc.feed(ref, 21, tail)
    again, _ = run(vio, pair, imu_handle, pnp_handle, 21, slid, feed=False)
    assert again["pnp_status"] == 0 and again["is_key"].tolist() == slid["is_key"] and again["n_frames"] == 15 and again["n_key"] == 11
    sc.feed(h, 22, slid)                                    # a never-used slot fed only the surviving and the new frames
    fresh = h.structure_batch([dict(slid["item"], slot=22)])[0]
    assert out_bytes(fresh) == out_bytes(again)
    a, b = h.frames_get(21), h.frames_get(22)               # the two differ in interval 0 alone, which structure does not read
    assert a["frames"][0]["exists"] == 1 and len(a["frames"][0]["dt"]) == 20 and b["frames"][0]["exists"] == 0 and len(b["frames"][0]["dt"]) == 0
    a["frames"][0].update({k: b["frames"][0][k] for k in ("exists", "first", "bias", "dt", "acc", "gyr")})
    assert ar.same_slot(a, b)


def test_a_try_that_fails_in_the_pnp_then_a_slide_then_a_good_try(vio, pair, imu_handle, pnp_handle):
    h, ref = pair
    base = sc.make("middle", seed=21)
    scene = sc.thin(base, 6, 5)                             # frame 6, the first of two non-keyframes in a row, sees five usable tracks
    got, _ = run(vio, pair, imu_handle, pnp_handle, 23, scene)
    assert (got["pnp_status"], got["fail_frame"]) == (FEW, 6) and np.isnan(h.frames_get(23)["frames"][6]["R"]).all() and np.isfinite(got["R"][7]).all()
    both(pair, "slide_batch", [(23, scene["frames"][6]["t"])])      # the failed frame leaves; the solved non-keyframe behind it leads now
    check(pair, [23])
    slid = sc.part(scene, 7, 15)
    again, _ = run(vio, pair, imu_handle, pnp_handle, 23, slid, feed=False)
    assert again["pnp_status"] == 0 and again["is_key"].tolist() == [0, 1, 1, 1, 1, 0, 1, 1] and np.isfinite(again["R"]).all() and np.isfinite(again["T"]).all()
    assert all(np.isfinite(f["R"]).all() and np.isfinite(f["T"]).all() for f in h.frames_get(23)["frames"])
    assert again["R"][[0, 5]].tobytes() == got["R"][[7, 12]].tobytes()          # the same frames from the same guesses
    # the same with the NaN rows staying in the window: an SfM that left most tracks dead, then one that did not
    item = base["item"]
    seen = np.isin(item["track_ids"], base["frames"][6]["ids"]) & (item["state"] != 0)
    few = np.zeros_like(item["state"])
    few[np.nonzero(seen)[0][:5]] = 1
    poor = dict(item, state=few, points=np.where(few[:, None] != 0, item["points"], np.nan))
    got, _ = run(vio, pair, imu_handle, pnp_handle, 24, base, item=poor)
    assert got["frame_status"][[2, 6, 7, 12]].tolist() == [FEW] * 4 and np.isnan(got["R"][[2, 6, 7, 12]]).all()
    both(pair, "slide_batch", [(24, base["frames"][1]["t"])])
    check(pair, [24])
    slid = sc.part(base, 2, 15)
    again, _ = run(vio, pair, imu_handle, pnp_handle, 24, slid, feed=False)
    assert again["pnp_status"] == 0 and np.isfinite(again["R"]).all() and np.isfinite(again["T"]).all() and again["is_key"].tolist() == base["is_key"][2:]
    assert all(np.isfinite(f["R"]).all() and np.isfinite(f["T"]).all() for f in h.frames_get(24)["frames"])


def test_a_failed_walk_a_reset_and_a_refused_image_leave_nothing_behind(vio, pair, imu_handle, pnp_handle):
    h, ref = pair
    front, full = sc.make("front", seed=5), sc.make("full", seed=4)
    # a try whose walk fails, then the good try: as on a fresh slot
    sc.feed(h, 25, front)
    sc.feed(ref, 25, front)
    hd = front["item"]["headers"]
    bad = h.structure_batch([dict(front["item"], slot=25, headers=np.concatenate([hd[:4], [hd[4] + 0.01], hd[5:]]))])[0]
    assert bad["status"] == ar.STATUS_WALK
    check(pair, [25])
    good, _ = run(vio, pair, imu_handle, pnp_handle, 25, front, feed=False)
    fresh, _ = run(vio, pair, imu_handle, pnp_handle, 26, front)
    assert good["pnp_status"] == 0 and out_bytes(good) == out_bytes(fresh) and ar.same_slot(h.frames_get(25), h.frames_get(26))
    # 32 frames structured, a reset, then the 12 frames of another scene: no is_key, R or T of the first window is left
    first, _ = run(vio, pair, imu_handle, pnp_handle, 27, full)
    assert first["n_frames"] == 32 and first["pnp_status"] == 0 and first["is_key"].tolist() == full["is_key"]
    # ... and a 33rd image is refused and changes nothing the next try sees
    f = front["frames"][0]
    r = both(pair, "imu_batch", [(27,) + f["samples"]])
    r = both(pair, "image_batch", [(27, 500.0, f["ids"], f["pts"], f["ba"], f["bg"])])
    assert r[0]["status"] == ar.STATUS_FRAMES_FULL and r[0]["n_frames"] == 32
    check(pair, [27])
    after = h.structure_batch([dict(full["item"], slot=27)])[0]
    assert out_bytes(after) == out_bytes(first)
    h.reset(27)
    ref.reset(27)
    check(pair, [27])
    reused, _ = run(vio, pair, imu_handle, pnp_handle, 27, front)
    assert out_bytes(reused) == out_bytes(fresh) and ar.same_slot(h.frames_get(27), h.frames_get(26))


# ---- f. initialize_from_frames ----
def test_initialize_from_frames_with_every_outcome_in_one_batch(vio, pair):
    h, ref = pair
    ih = vio.load_init().create()
    good_a, good_b, thin = sc.make("middle", seed=6), sc.make("front", seed=5), sc.thin(sc.make("middle", seed=21), 2, 5)
    scenes = {50: good_a, 51: good_b, 52: good_b, 53: good_b, 54: thin}       # good, SfM failed, walk failed, good, PnP failed
    for s, scn in scenes.items():
        sc.feed(h, s, scn)
    sfm_of = lambda scn: dict(status=0, Q=scn["item"]["Q"], T=scn["item"]["T"], points=scn["item"]["points"], state=scn["item"]["state"])
    hd = good_b["item"]["headers"]
    moved = np.concatenate([hd[:4], [hd[4] + 0.01], hd[5:]])
    sfm = [sfm_of(good_a), dict(status=3), sfm_of(good_b), sfm_of(good_b), sfm_of(thin)]
    headers = [good_a["item"]["headers"], None, moved, hd, thin["item"]["headers"]]
    ids = [good_a["item"]["track_ids"], None, good_b["item"]["track_ids"], good_b["item"]["track_ids"], thin["item"]["track_ids"]]
    try:
        out = vio.initialize_from_frames(vio.BatchImageFrames(h, list(scenes)), ih, sfm, headers, ids, sc.RIC, sc.TIC, 9.81)
        assert [o is None for o in out] == [False, True, True, False, True]
        two = vio.initialize_from_frames(vio.BatchImageFrames(h, [50, 53]), ih, [sfm[0], sfm[3]], [headers[0], headers[3]], [ids[0], ids[3]], sc.RIC, sc.TIC, 9.81)
        for o, w, scn in zip((out[0], out[3]), two, (good_a, good_b)):
            assert o["status"] == w["status"] == 0 and o["n_key"] == 11 and o["structure"]["is_key"].tolist() == scn["is_key"]
            assert abs(o["s"] - sc.SCALE) < 0.05 * sc.SCALE and np.abs(o["g"] - sc.GRAVITY).max() < 0.1 and np.abs(o["bg"] - sc.BG_TRUE).max() < 0.005
            for k in ("s", "g", "g_world", "s_linear", "g_linear", "bg", "poses", "speed_bias", "x", "rot"):
                assert np.isfinite(o[k]).all() and np.asarray(o[k]).tobytes() == np.asarray(w[k]).tobytes(), k
            assert out_bytes(o["structure"]) == out_bytes(w["structure"])
            assert all(np.array_equal(a[k], b[k]) for a, b in zip(o["pre"], w["pre"]) for k in ("delta_p", "delta_q", "delta_v", "jacobian", "covariance"))
    finally:
        ih.close()


# ---- g. the argument rules of vio_aif_structure_batch ----
def test_argument_errors_of_structure_write_nothing_and_leave_both_slots(vio, lib, pair):
    h, ref = pair
    scene, other = sc.make("front", seed=5), sc.limit_scene("nkk257")
    sc.feed(h, 60, scene)
    sc.feed(h, 61, other)
    before = [h.frames_get(60), h.frames_get(61)]
    good, item = dict(scene["item"], slot=60), dict(other["item"], slot=61)
    twice = item["track_ids"].copy()
    twice[200] = twice[3]
    hd_nan, ric_inf = item["headers"].copy(), np.array(item["ric"], dtype=np.float64)
    hd_nan[1] = np.nan
    ric_inf[1, 2] = np.inf
    cases = [("n_key 0", dict(item, n_key=0), None, "item 1"), ("n_key 33", dict(item, n_key=33), None, "item 1"),
             ("n_tracks 4097", dict(item, n_tracks=4097), None, "item 1"), ("a track id twice", dict(item, track_ids=twice), None, "item 1"),
             ("NULL headers", item, "headers", "item 1"), ("NULL track_ids", item, "track_ids", "item 1"), ("NULL R", item, "R", "item 1"),
             ("a slot twice", dict(item, slot=60), None, "item 1"), ("slot 256", dict(item, slot=256), None, "item 1"),
             ("a non-finite header", dict(item, headers=hd_nan), None, "item 1"), ("a non-finite ric", dict(item, ric=ric_inf), None, "item 1")]
    for name, bad, null, said in cases:
        st, untouched, _, _ = raw_call(lib, h, [good, bad], null={1: (null,)} if null else None)
        assert st == -1 and untouched, name
        assert said in h.last_error(), (name, h.last_error())
        assert ar.same_slot(h.frames_get(60), before[0]) and ar.same_slot(h.frames_get(61), before[1]), name
    st, untouched, _, _ = raw_call(lib, h, [good, item], count=257)
    assert st == -1 and untouched and "count 257" in h.last_error()
    st, untouched, _, _ = raw_call(lib, h, [good, item], count=-1)
    assert st == -1 and untouched
    st, untouched, _, _ = raw_call(lib, h, [good, item], count=0)
    assert st == 0 and untouched and h.structure_batch([]) == []
    assert ar.same_slot(h.frames_get(60), before[0]) and ar.same_slot(h.frames_get(61), before[1])
    with pytest.raises(vio.VioError) as e:                  # through the binding: the status and the item
        h.structure_batch([good, dict(item, track_ids=twice)])
    assert e.value.status == -1 and "item 1" in str(e.value)
    # the handle is unharmed: the same call without the mistake is the two items alone
    st, untouched, res, outs = raw_call(lib, h, [good, item])
    assert st == 0 and not untouched and [r.status for r in res] == [0, 0] and [r.pnp_status for r in res] == [0, 0]
    alone = [h.structure_batch([good])[0], h.structure_batch([item])[0]]
    for o, a in zip(outs, alone):
        F = a["n_frames"]
        assert o["R"][:F].tobytes() == a["R"].tobytes() and o["T"][:F].tobytes() == a["T"].tobytes() and o["is_key"][:F].tolist() == a["is_key"].tolist()
        assert np.all(o["R"][F:] == 7.5) and np.all(o["T"][F:] == 7.5) and np.all(o["is_key"][F:] == 77)      # nothing behind n_frames
