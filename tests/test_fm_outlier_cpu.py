"""vio_fm_remove_batch without a device.  csrc/vio_fm_outlier_math.h (the bisection k_fm_remove runs, the host's sort with its
permutation and duplicate check) compiled with tests/cpp/fm_outlier_main.cpp into a stand-alone program (ASan and UBSan with
VIO_TEST_SANITIZE=1; never loaded into Python) against numpy's searchsorted.  And the drivers' wiring on the CPU oracle backend with
the residual query replaced by a function of the window alone, so that the dict path and the slot path are told the same thing:
StreamDriver(features=(NumpyFmOutlier, slot), outlier_px=) beside the dict-path driver, and run_batched over three such drivers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fm_outlier_reference as fo
import fm_stream_reference as fsr
from stream_group_util import OracleMarg, patch_batched, stub_driver
from test_fm_stream_cpu import STREAMS, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("fm_outlier")
    exe = d / "fm_outlier"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if os.environ.get("VIO_TEST_SANITIZE") == "1" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "fm_outlier_main.cpp")])
    return d, str(exe)


def query(driver, cases):
    """cases: (ids, keys); per case (distinct, perm, lower_bound, find, erased)."""
    d, exe = driver
    fin, fout = str(d / "in.txt"), str(d / "out.txt")
    with open(fin, "w") as f:
        for ids, keys in cases:
            f.write("Q %d %s %d %s\n" % (len(ids), " ".join(str(int(v)) for v in ids), len(keys), " ".join(str(int(v)) for v in keys)))
    subprocess.check_call([exe, fin, fout])
    lines = [ln.split() for ln in open(fout).read().splitlines()]
    assert len(lines) == len(cases)
    out = []
    for (ids, keys), ln in zip(cases, lines):
        n, m = len(ids), len(keys)
        v = [int(x) for x in ln[1:]]
        assert ln[0] == "Q" and len(v) == 1 + 2 * n + 2 * m
        out.append((v[0], np.array(v[1:1 + n], dtype=np.int64), np.array(v[1 + n:1 + n + m], dtype=np.int64),
                    np.array(v[1 + n + m:1 + n + 2 * m], dtype=np.int64), np.array(v[1 + n + 2 * m:], dtype=np.int64)))
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2048])
def test_bisection_and_sort_against_searchsorted(driver, n):
    rng = np.random.RandomState(100 + n)
    spreads = [rng.choice(np.arange(-3 * n - 5, 3 * n + 5, dtype=np.int64), size=n, replace=False),        # dense: many keys hit
               rng.randint(I64_MIN + 1, I64_MAX, size=n, dtype=np.int64)]                                      # the whole range
    if n >= 2:
        ext = spreads[1].copy()
        ext[0], ext[-1] = I64_MAX, I64_MIN                # the extremes as ids, out of order
        spreads.append(ext)
    cases = []
    for ids in spreads:
        ids = np.unique(ids)
        rng.shuffle(ids)
        s = np.sort(ids)
        keys = [I64_MIN, I64_MAX, 0, -1]
        if len(s):
            keys += [int(s[0]), int(s[-1]), int(s[len(s) // 2])]
            keys += [int(s[0]) - 1] if s[0] > I64_MIN else []                 # below all
            keys += [int(s[-1]) + 1] if s[-1] < I64_MAX else []               # above all
            keys += [int(v) for v in rng.choice(s, size=min(len(s), 40), replace=False)]
            keys += [int(v) + 1 for v in rng.choice(s, size=min(len(s), 20), replace=False) if v < I64_MAX]
        cases.append((ids, np.array(keys, dtype=np.int64)))
    for (ids, keys), (distinct, perm, lb, find, erased) in zip(cases, query(driver, cases)):
        s = np.sort(ids)
        assert distinct == 1
        assert np.array_equal(ids[perm], s) if len(ids) else len(perm) == 0
        assert np.array_equal(lb, np.searchsorted(s, keys, side="left"))
        hit = np.isin(keys, s)
        assert np.array_equal(find >= 0, hit) and np.array_equal(s[find[hit]], keys[hit])
        assert np.array_equal(erased.astype(bool), np.isin(ids, keys))


def test_duplicate_ids_are_found_wherever_they_stand(driver):
    base = np.array([5, -3, 2 ** 40, I64_MIN, 9, I64_MAX, 0], dtype=np.int64)
    big = np.arange(2048, dtype=np.int64)[::-1].copy()
    dup_big = big.copy()
    dup_big[2047] = dup_big[0]
    cases = [(base, []), (np.append(base, 5), []), (np.append(base, I64_MIN), []), (np.append(base, I64_MAX), []), (np.array([7, 7]), []),
             (big, []), (dup_big, [])]
    got = [g[0] for g in query(driver, cases)]
    assert got == [1, 0, 0, 0, 0, 1, 0]


# ---- the drivers' wiring ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nonkey,n_frames", STREAMS)
def test_slot_path_rejects_what_the_dict_path_rejects(vio, oracle_lib, seed, nonkey, n_frames):
    vs = vio.stream
    plain = stub_driver(vs.StreamDriver(oracle_lib, make(vs, seed, n_frames), triangulate=True, nonkey_every=nonkey, outlier_px=3.0))
    want = fsr.record_dict_driver(plain)
    fm = fsr.Recording(fo.NumpyFmOutlier(plain.ctx.triangulate))
    drv = stub_driver(vs.StreamDriver(oracle_lib, make(vs, seed, n_frames), triangulate=True, nonkey_every=nonkey, outlier_px=3.0, features=(fm, 3)))
    assert not hasattr(drv, "tracks") and not hasattr(drv, "depth")
    tp, td = plain.run(), drv.run()
    got = fm.exports[3]
    assert len(got) == len(want) == 2 * len(tp) == 2 * len(td)
    for step, (g, w) in enumerate(zip(got, want)):
        for k in ("feature_ids", "lm", "host", "target", "pts_i", "pts_j"):
            assert g[k].dtype == w[k].dtype and np.array_equal(g[k], w[k]), (step, k)
    assert drv.rejected == plain.rejected and drv.rejected_ids == plain.rejected_ids
    assert sum(drv.rejected) > 10 and len(set(drv.rejected_ids)) == len(drv.rejected_ids)
    assert drv.fm_erased == drv.rejected and plain.fm_erased == []      # (remove_failures is off: every flagged id still had its row)
    assert [c for c in fm.calls if c[0] == "remove_batch"] == [("remove_batch", 1)] * len(td)
    # no rejected id is in any later export: step s rejects from export 2 s; the exports from 2 s + 2 on come after its erase
    at = 0
    for s, n in enumerate(drv.rejected):
        gone = set(drv.rejected_ids[at:at + n])
        at += n
        assert gone <= set(int(i) for i in got[2 * s]["feature_ids"])
        for later in got[2 * s + 2:]:
            assert not gone & set(int(i) for i in later["feature_ids"])
    assert np.array_equal(drv.have_depth, plain.have_depth)


def test_an_id_remove_failures_took_counts_as_rejected_and_not_as_erased(vio, oracle_lib):
    """remove_failures=True erases the rows solved to a negative depth in front of the erase by id: such an id is in rejected and
    rejected_ids, and remove_batch finds no row for it."""
    vs = vio.stream

    class Fm(fo.NumpyFmOutlier):
        def set_depth_batch(self, items, mode=0, remove_failures=False):
            items = [(s, np.where(np.arange(len(x)) % 7 == 3, -np.abs(x), x)) for s, x in items]     # the stub's bit-0 landmarks fail
            return fo.NumpyFmOutlier.set_depth_batch(self, items, mode, remove_failures)
    d0 = vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True)
    fm = fsr.Recording(Fm(d0.ctx.triangulate))
    drv = stub_driver(vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True, outlier_px=3.0,
                                      features=dict(handle=fm, slot=1, remove_failures=True)))
    drv.step()
    k = np.arange(len(fm.exports[1][0]["feature_ids"]))
    assert drv.rejected == [int(((k % 7 == 3) | (k % 11 == 5)).sum())]
    assert drv.fm_erased == [int(((k % 11 == 5) & (k % 7 != 3)).sum())] and 0 < drv.fm_erased[0] < drv.rejected[0]
    _, ids = vs.fm_windows([drv], False)[0]
    assert not set(drv.rejected_ids) & set(ids)


def batch_group(vio, oracle_lib, monkeypatch, thresholds, fm):
    from vio_amd import batch_stream
    vs = vio.stream
    seen = patch_batched(monkeypatch, oracle_lib)
    drivers = []
    for k, ((seed, nonkey, n_frames), px) in enumerate(zip(STREAMS, thresholds)):
        d = vs.StreamDriver(oracle_lib, make(vs, seed, n_frames), triangulate=True, nonkey_every=nonkey, outlier_px=px, features=(fm, 10 + k))
        d.ctx.get_stream = lambda: None                 # (the CPU backend has no stream to share)
        drivers.append(d)
    trajs = batch_stream.run_batched(drivers, OracleMarg(oracle_lib))
    return drivers, trajs, seen


def test_run_batched_makes_one_remove_batch_per_frame(vio, oracle_lib, monkeypatch):
    vs = vio.stream
    tri = oracle_lib.context().triangulate
    fm = fsr.Recording(fo.NumpyFmOutlier(tri))
    drivers, trajs, seen = batch_group(vio, oracle_lib, monkeypatch, (3.0, None, 3.0), fm)
    frames = [len(t) for t in trajs]
    with_px = [sum(f > i for f, d in zip(frames, drivers) if d.outlier_px is not None) for i in range(max(frames))]
    assert [n for c, n in fm.calls if c == "remove_batch"] == [n for n in with_px if n]
    assert seen == [(n, 3.0, ("flags",)) for n in with_px if n]
    assert drivers[1].rejected == [] and drivers[1].rejected_ids == [] and drivers[1].fm_erased == []
    for d in (drivers[0], drivers[2]):
        assert len(d.rejected) == len(d.trajectory) and sum(d.rejected) > 10 and d.fm_erased == d.rejected
        at = 0
        got = fm.exports[d.fm_slot]
        for s, n in enumerate(d.rejected):
            gone = set(d.rejected_ids[at:at + n])
            at += n
            assert gone <= set(int(i) for i in got[2 * s]["feature_ids"])
            for later in got[2 * s + 2:]:
                assert not gone & set(int(i) for i in later["feature_ids"])
    # the driver without a threshold: the exports of its run alone
    seed, nonkey, n_frames = STREAMS[1]
    solo_fm = fsr.Recording(fo.NumpyFmOutlier(tri))
    solo = vs.StreamDriver(oracle_lib, make(vs, seed, n_frames), triangulate=True, nonkey_every=nonkey, features=(solo_fm, 0))
    ts = solo.run()
    assert ts.shape == trajs[1].shape
    a, b = solo_fm.exports[0], fm.exports[11]
    assert len(a) == len(b)
    for step, (g, w) in enumerate(zip(b, a)):
        for k in ("feature_ids", "lm", "host", "target", "pts_i", "pts_j"):
            assert np.array_equal(g[k], w[k]), (step, k)


def test_run_batched_groups_the_query_by_threshold(vio, oracle_lib, monkeypatch):
    fm = fsr.Recording(fo.NumpyFmOutlier(oracle_lib.context().triangulate))
    drivers, trajs, seen = batch_group(vio, oracle_lib, monkeypatch, (3.0, 5.0, 3.0), fm)
    first = seen[:2]
    assert first == [(2, 3.0, ("flags",)), (1, 5.0, ("flags",))]
    assert [n for c, n in fm.calls if c == "remove_batch"][0] == 3


def test_refusals(vio, oracle_lib):
    from vio_amd import batch_stream
    vs = vio.stream
    with pytest.raises(ValueError, match="outlier_px"):      # a handle without remove_batch
        vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True, outlier_px=3.0, features=(fsr.NumpyFm(None), 0))
    with pytest.raises(ValueError, match="outlier_px"):
        vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True, outlier_px=3.0, features=(fsr.Recording(fsr.NumpyFm(None)), 0))
    d = vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True, outlier_px=3.0)     # no features=
    d.ctx.get_stream = lambda: None
    with pytest.raises(ValueError, match="outlier_px"):
        batch_stream.run_batched([d], None)
    ok = vs.StreamDriver(oracle_lib, make(vs, 0, 13), triangulate=True, outlier_px=3.0, features=(fo.NumpyFmOutlier(oracle_lib.context().triangulate), 0))
    ok.ctx.get_stream = lambda: None
    batch_stream._check([ok])
