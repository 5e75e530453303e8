"""vio_fm_remove_batch (include/vio_fm_outlier.h) on the device against tests/fm_outlier_reference.py's
remove_ids: the rows that stay byte for byte (ids, starts, the depths' bit patterns, flags, offsets, points), the three counts, n_rows
and erased.  Tables are seeded with tracks_set and read with tracks_get.  Shapes: the wavefront edges of the ballot scan (63, 64, 65),
the chunk edge of FM_NT (1023, 1024, 1025) and the full table (2047, 2048).  Then the drivers: StreamDriver(features=, outlier_px=) and
run_batched on the corrupted stream of tests/test_gpu_residuals.py."""
import ctypes as C

import numpy as np
import pytest

import fm_outlier_reference as fo
import fm_reference as fr
import fm_stream_reference as fsr

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048]
BAD_ARG = -1
FIELDS = ("ids", "start", "depth", "flag", "off", "pts")


@pytest.fixture(scope="module")
def fh(vio):
    h = vio.load_fm().create()                           # (a missing library raises: a failure, not a skip)
    yield h
    h.close()


def make_rows(n, seed=0):
    """n rows, n_obs cycling 1 .. 11; an even row starts early (usable where n_obs >= 2), an odd row as late as its observations
    allow (not usable where n_obs <= 3): usable and unusable rows stand side by side all along the table.  Ids above 2^31, distinct,
    not sorted; depths unknown (-1), positive and negative; flags 0, 1, 2."""
    rng = np.random.RandomState(1000 + 7 * n + seed)
    ids = rng.permutation(n).astype(np.int64) * 2500013 + 2 ** 31 + 11 + seed
    out = []
    for i in range(n):
        k = 1 + i % 11
        start = i % min(8, 12 - k) if i % 2 == 0 else 11 - k
        depth = (-1.0, float(rng.uniform(2.0, 9.0)), -float(rng.uniform(0.5, 3.0)))[i % 3]
        out.append(dict(id=int(ids[i]), start=start, depth=depth, flag=(i // 3) % 3, pts=rng.uniform(-0.7, 0.7, (k, 2))))
    return out


def patterns(tracks, seed=0):
    n = len(tracks)
    ids = np.array([t["id"] for t in tracks], dtype=np.int64)
    rng = np.random.RandomState(seed + n)
    absent = np.array([-5, 7, 2 ** 31 + 10, 2 ** 62, -2 ** 63, 2 ** 63 - 1], dtype=np.int64)
    assert not np.isin(absent, ids).any()
    edge = [1023, 1024] if n >= 1025 else [r for r in (n // 2 - 1, n // 2) if 0 <= r < n]      # astride the chunk edge where there is one
    mixed = np.concatenate([ids[::3][::-1], absent])
    mixed = mixed[np.argsort(rng.uniform(size=len(mixed)), kind="stable")] if n % 2 else np.concatenate([absent[:3], ids[::3][::-1], absent[3:]])
    return [("none", ids[:0]), ("all", ids.copy()), ("first", ids[:1]), ("last", ids[n - 1:]), ("edge", ids[np.array(edge, dtype=np.int64)]), ("every other", ids[::2]),
            ("a third", ids[rng.uniform(size=n) < 1.0 / 3.0]), ("all but one", np.delete(ids, n // 2) if n else ids[:0]),
            ("reversed with absent ids", mixed)]


def seed_slot(fh, slot, tracks):
    fh.tracks_set(slot, *fr.tracks_to_arrays(tracks))
    assert fh.counts(slot) == fr.counts(tracks)


def assert_bytes(got, want):
    """Two tracks_get dicts byte for byte."""
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def check(fh, slot, tracks, ids, res):
    want, erased = fo.remove_ids(tracks, ids)
    assert_bytes(fh.tracks_get(slot), fsr.tracks_arrays(want))
    assert (res["n_tracks"], res["n_landmarks"], res["n_observations"]) == fr.counts(want) == fh.counts(slot)
    assert res["status"] == 0 and res["n_rows"] == len(tracks) - len(want) == int(erased.sum())
    assert res["erased"].dtype == bool and np.array_equal(res["erased"], erased)
    assert [res[k] for k in ("keyframe", "last_track_num", "parallax_num", "n_new", "n_triangulated", "parallax_sum")] == [0] * 6
    return want


@pytest.mark.parametrize("n", ROWS)
def test_remove_matches_the_restatement(fh, n):
    tracks = make_rows(n)
    for name, ids in patterns(tracks):
        seed_slot(fh, 0, tracks)
        res = fh.remove_batch([(0, ids)])[0]
        want = check(fh, 0, tracks, ids, res)
        image = fh.tracks_get(0)
        again = fh.remove_batch([(0, ids)])[0]               # a second identical call erases nothing and leaves the bytes
        assert again["n_rows"] == 0 and not again["erased"].any(), name
        assert_bytes(fh.tracks_get(0), image)
        assert (again["n_tracks"], again["n_landmarks"], again["n_observations"]) == fr.counts(want)


def test_failed_rows_by_id_leave_what_remove_failures_leaves(fh):
    """set_depth_batch(remove_failures=True) in one slot; in its twin set_depth_batch without, then remove_batch with the ids of the
    solve_flag == 2 rows: the same bytes."""
    tracks = make_rows(1500, seed=3)
    x = np.linspace(0.1, 0.6, fr.counts(tracks)[1])
    x[::5] *= -1.0
    seed_slot(fh, 1, tracks)
    seed_slot(fh, 2, tracks)
    fh.set_depth_batch([(1, x)], remove_failures=True)
    fh.set_depth_batch([(2, x)], remove_failures=False)
    tw = fh.tracks_get(2)
    ids = tw["ids"][tw["flag"] == 2]
    assert len(ids) >= len(x[::5])
    res = fh.remove_batch([(2, ids)])[0]
    assert res["erased"].all() and res["n_rows"] == len(ids)
    assert_bytes(fh.tracks_get(2), fh.tracks_get(1))
    assert fh.counts(2) == fh.counts(1)


def test_an_erased_id_comes_back_as_a_new_row(vio, fh):
    from test_gpu_fm import poses_of
    tracks = make_rows(1025, seed=5)
    seed_slot(fh, 4, tracks)
    gone = np.array([tracks[500]["id"], tracks[1024]["id"], tracks[3]["id"]], dtype=np.int64)
    res = fh.remove_batch([(4, gone)])[0]
    want = check(fh, 4, tracks, gone, res)
    ids = np.array([tracks[500]["id"], 2 ** 40 + 9], dtype=np.int64)
    pts = np.array([[0.125, -0.25], [0.5, 0.0625]])
    want, r = fr.add(want, 10, ids, pts)
    got = fh.add_batch([(4, 10, ids, pts)])[0]
    assert got["status"] == 0 and got["n_new"] == r["n_new"] == 2 and got["last_track_num"] == 0
    assert len(want) == 1024 and want[-2]["id"] == tracks[500]["id"] and len(want[-2]["pts"]) == 1
    assert_bytes(fh.tracks_get(4), fsr.tracks_arrays(want))
    poses, ext = poses_of(vio)
    exp = fh.export_batch([(4, poses, ext)], triangulate=False)[0]
    ref = fr.export(want)
    for k in fsr.WINDOW_FIELDS:
        assert exp[k].dtype == ref[k].dtype and exp[k].tobytes() == ref[k].tobytes(), k


def test_five_slots_in_one_call(fh):
    """Sizes 0 (a slot never used), 5, 64, 1025 and 2048, one item without ids: every slot as alone, and as in other slot indices."""
    lists = [[], make_rows(5, 1), make_rows(64, 2), make_rows(1025, 3), make_rows(2048, 4)]
    erase = [np.array([9, 2 ** 33], dtype=np.int64), patterns(lists[1])[5][1], np.zeros(0, dtype=np.int64), patterns(lists[3])[8][1], patterns(lists[4])[6][1]]

    def run(slots, batch):
        for s, tr in zip(slots, lists):
            if tr or s != 251:                           # (251 is used nowhere else: never allocated)
                seed_slot(fh, s, tr)
        if batch:
            res = fh.remove_batch(list(zip(slots, erase)))
        else:
            res = [fh.remove_batch([(s, e)])[0] for s, e in zip(slots, erase)]
        return res, [fh.tracks_get(s) for s in slots]
    res0, img0 = run([251, 3, 17, 200, 255], True)
    for tr, e, r, img in zip(lists, erase, res0, img0):
        want, erased = fo.remove_ids(tr, e)
        assert_bytes(img, fsr.tracks_arrays(want))
        assert r["n_rows"] == int(erased.sum()) and np.array_equal(r["erased"], erased)
    for slots, batch in (([100, 101, 102, 103, 104], False), ([255, 200, 0, 3, 17], True)):
        res, img = run(slots, batch)
        for a, b, ia, ib in zip(res0, res, img0, img):
            assert {k: v for k, v in a.items() if k != "erased"} == {k: v for k, v in b.items() if k != "erased"}
            assert np.array_equal(a["erased"], b["erased"])
            assert_bytes(ib, ia)
    from vio_amd.fm import BatchFeatureManager
    for s, tr in zip([100, 101, 102, 103, 104], lists):
        seed_slot(fh, s, tr)
    bfm_res = BatchFeatureManager(fh, [100, 101, 102, 103, 104]).remove(erase)
    assert [r["n_rows"] for r in bfm_res] == [r["n_rows"] for r in res0]


def test_argument_errors_write_nothing(vio, fh):
    """Past the binding's own checks, on the library: BAD_ARG, the message names the item, no table and no result changes."""
    Item, Result = vio.fm.VioFmRemoveItem, vio.fm.VioFmResult
    lists = {7: make_rows(70, 8), 8: make_rows(1030, 9)}
    for s, tr in lists.items():
        seed_slot(fh, s, tr)
    before = {s: fh.tracks_get(s) for s in lists}
    ok = np.array([lists[7][0]["id"], lists[7][5]["id"]], dtype=np.int64)
    dup = np.array([lists[8][1]["id"], 5, lists[8][1]["id"]], dtype=np.int64)
    many = np.arange(2049, dtype=np.int64)
    erased = np.full(2049, 9, dtype=np.uint8)
    p = lambda a: a.ctypes.data                           # noqa: E731
    cases = [("listed twice", "item 1", [Item(7, 2, p(ok), p(erased)), Item(8, 3, p(dup), p(erased))]),
             ("listed twice", "item 1", [Item(7, 2, p(ok), p(erased)), Item(7, 2, p(ok), p(erased))]),
             ("n = 2049", "item 1", [Item(7, 2, p(ok), p(erased)), Item(8, 2049, p(many), p(erased))]),
             ("n = -1", "item 0", [Item(7, -1, p(ok), p(erased))]),
             ("ids is required", "item 1", [Item(7, 2, p(ok), p(erased)), Item(8, 2, None, p(erased))]),
             ("slot", "item 0", [Item(256, 2, p(ok), p(erased))])]
    fn = fh.lib.fn["remove_batch"]
    for text, item, items in cases:
        arr = (Item * len(items))(*items)
        res = (Result * len(items))()
        C.memset(res, 0x5A, C.sizeof(res))
        assert fn(fh.h, C.c_int32(len(items)), C.addressof(arr), C.addressof(res)) == BAD_ARG, text
        msg = fh.last_error()
        assert text in msg and item in msg and "vio_fm_remove_batch" in msg, msg
        assert bytes(res) == b"\x5a" * C.sizeof(res) and (erased == 9).all()
        for s in lists:
            assert_bytes(fh.tracks_get(s), before[s])
            assert fh.counts(s) == fr.counts(lists[s])
    res = (Result * 1)()
    arr = (Item * 1)(Item(7, 0, None, None))
    assert fn(fh.h, C.c_int32(257), C.addressof(arr), C.addressof(res)) == BAD_ARG and "count" in fh.last_error()
    assert fn(fh.h, C.c_int32(-1), C.addressof(arr), C.addressof(res)) == BAD_ARG
    assert fn(fh.h, C.c_int32(1), None, C.addressof(res)) == BAD_ARG and fn(fh.h, C.c_int32(1), C.addressof(arr), None) == BAD_ARG
    assert fn(fh.h, C.c_int32(0), None, None) == 0
    assert fn(fh.h, C.c_int32(1), C.addressof(arr), C.addressof(res)) == 0 and res[0].n_rows == 0 and res[0].n_tracks == 70      # n == 0 with NULL ids
    with pytest.raises(vio.VioError) as e:
        fh.remove_batch([(7, ok), (7, ok)])
    assert e.value.status == BAD_ARG and "listed twice" in str(e.value)
    for s in lists:
        assert_bytes(fh.tracks_get(s), before[s])


# ------------------------------------------------ drivers -----------------------------------------------------------------
class Spy(fsr.Recording):
    """Recording, and per remove_batch call and item: the ids, the slot's list before and after, the result."""

    def __init__(self, handle):
        fsr.Recording.__init__(self, handle)
        self.removes = []

    def remove_batch(self, items):
        before = [self._h.tracks_get(s) for s, _ in items]
        res = self._h.remove_batch(items)
        self.calls.append(("remove_batch", len(items)))
        self.removes.append([dict(slot=int(s), ids=np.array(ids, dtype=np.int64), before=b, after=self._h.tracks_get(s), res=r)
                             for (s, ids), b, r in zip(items, before, res)])
        return res


def check_steps(vio, d, fm, queries, bad):
    """One driver's run: what the issue's step-by-step checks ask, and recall / precision against the planted set."""
    mine = [rm for call in fm.removes for rm in call if rm["slot"] == d.fm_slot]
    exports = fm.exports[d.fm_slot]
    assert len(mine) == len(queries) == len(d.rejected) == len(d.trajectory) and len(exports) == 2 * len(mine)
    seen, at = set(), 0
    for s, (rm, (w, flags)) in enumerate(zip(mine, queries)):
        first = exports[2 * s]
        seen |= set(int(i) for i in first["feature_ids"])
        assert np.array_equal(w.lm, first["lm"]) and np.array_equal(w.pts_j, first["pts_j"])        # the query ran on that window
        want_ids = first["feature_ids"][(flags & 7) != 0]
        assert np.array_equal(rm["ids"], want_ids), s
        assert d.rejected[s] == len(want_ids) and d.rejected_ids[at:at + len(want_ids)] == [int(i) for i in want_ids]
        at += len(want_ids)
        kept, erased = fo.remove_ids(fr.arrays_to_tracks(rm["before"]), rm["ids"])
        assert_bytes(rm["after"], fsr.tracks_arrays(kept))
        assert rm["res"]["n_rows"] == int(erased.sum()) == d.fm_erased[s] and np.array_equal(rm["res"]["erased"], erased)
        for later in exports[2 * s + 2:]:
            assert not np.isin(later["feature_ids"], want_ids).any(), s
    rejected = set(d.rejected_ids)
    assert len(rejected) == len(d.rejected_ids)
    solved_bad = bad & seen
    recall = len(rejected & solved_bad) / max(1, len(solved_bad))
    precision = len(rejected & bad) / max(1, len(rejected))
    print("slot %d: %d corrupted tracks solved, %d rejected (recall %.3f, precision %.3f)" % (d.fm_slot, len(solved_bad), len(rejected), recall, precision))
    assert len(solved_bad) > 0 and recall >= 0.5 and precision >= 0.5, (recall, precision)


def test_driver_erases_what_the_residual_query_flags(vio, hip_lib, fh):
    from test_gpu_residuals import _corrupted_stream
    st, bad = _corrupted_stream(vio)
    fm = Spy(fh)
    d = vio.stream.StreamDriver(hip_lib, st, triangulate=True, outlier_px=3.0, features=(fm, 30))
    queries, inner = [], d.ctx.residuals

    def residuals(w, focal=None, outlier_px=3.0):
        r = inner(w, focal, outlier_px)
        again = inner(w, focal, outlier_px)                  # recomputed on that window: the same flags
        assert outlier_px == 3.0 and np.array_equal(r["flags"], again["flags"])
        queries.append((w, r["flags"].copy()))
        return r
    d.ctx.residuals = residuals
    traj = d.run()
    assert np.isfinite(traj).all() and fm.calls.count(("remove_batch", 1)) == len(traj)
    check_steps(vio, d, fm, queries, bad)


@pytest.mark.parametrize("with_state", [False, True])
def test_run_batched_erases_in_one_call_per_frame(vio, hip_lib, fh, monkeypatch, with_state):
    """with_state: the drivers' window states live in estimator-state slots as well (state=), the other order of slide in
    step_batched."""
    from test_gpu_residuals import _corrupted_stream
    from vio_amd import batch_stream
    vs = vio.stream
    inner = hip_lib.batch_residuals
    queries = {}

    def batch_residuals(ctxs, windows, focal=None, outlier_px=3.0, outputs=None):
        res = inner(ctxs, windows, focal=focal, outlier_px=outlier_px, outputs=outputs)
        assert outputs == ("flags",) and outlier_px == 3.0
        for c, w, r in zip(ctxs, windows, res):                 # the batch is bitwise the single call on that window
            single = c.residuals(w, outlier_px=outlier_px)
            assert np.array_equal(single["flags"], r["flags"])
            queries.setdefault(id(c), []).append((w, r["flags"].copy()))
        return res
    monkeypatch.setattr(hip_lib, "batch_residuals", batch_residuals, raising=False)

    def group(fm, who):
        ds, sh = [], None
        for k, (seed, px) in enumerate(((1, 3.0), (2, 3.0), (1, None))):
            if k not in who:
                continue
            st, bad = _corrupted_stream(vio)
            kw = dict(ctx_kwargs=dict(stream=sh)) if sh is not None else {}
            if est is not None:
                kw["state"] = (est, 7 + 90 * k)
            ds.append(vs.StreamDriver(hip_lib, st, seed=seed, triangulate=True, outlier_px=px, features=(fm, 40 + 60 * k), **kw))
            sh = ds[0].ctx.get_stream()
        return ds, batch_stream.run_batched(ds, vio.load_marg().create(stream=sh)), bad
    est = vio.load_est().create() if with_state else None
    try:
        fm = Spy(fh)
        ds, trajs, bad = group(fm, (0, 1, 2))
        assert [n for c, n in fm.calls if c == "remove_batch"] == [2] * len(trajs[0])
        for d in ds[:2]:
            check_steps(vio, d, fm, queries[id(d.ctx)], bad)
        assert ds[2].rejected == [] and ds[2].fm_erased == [] and id(ds[2].ctx) not in queries
        alone, ta, _ = group(Spy(fh), (2,))
        assert np.array_equal(ta[0], trajs[2])
    finally:
        if est is not None:
            est.close()
