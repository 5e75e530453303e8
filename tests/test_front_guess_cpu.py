"""The prediction's rule without a device.  csrc/vio_front_guess_math.h (front_guess_normalise, front_guess_find,
front_guess_falls_back), the text vio_frame.hip and the kernels of csrc/vio_front_guess_body.inc call, compiled into the stand-alone
program tests/cpp/front_guess_main.cpp (its own main; ASan and UBSan with VIO_TEST_SANITIZE=1; never loaded into Python) against
tests/front_guess_reference.py, the numpy restatement of frontend.FeatureTracker._take_guess: the uploaded rows, the row found per
point, the composed guess and n_guessed bit for bit, and the fallback's decision at its boundary."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_guess_reference as fg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
I64 = np.iinfo(np.int64)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("front_guess")
    exe = d / "front_guess"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if os.environ.get("VIO_TEST_SANITIZE") == "1" else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "front_guess_main.cpp")])
    return d, str(exe)


def host(driver, ids, cur, pred_ids, pred_px, cases=()):
    d, exe = driver
    ids, pred_ids = np.asarray(ids, np.int64).reshape(-1), np.asarray(pred_ids, np.int64).reshape(-1)
    cur, pred_px = np.asarray(cur, np.float32).reshape(-1, 2), np.asarray(pred_px, np.float32).reshape(-1, 2)
    cases = np.asarray(cases, np.int32).reshape(-1, 3)
    n, p, c = len(ids), len(pred_ids), len(cases)
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", n, p, c) + ids.tobytes() + cur.tobytes() + pred_ids.tobytes() + pred_px.tobytes() + cases.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    m = struct.unpack_from("<i", raw)[0]
    assert len(raw) == 4 + 16 * m + 12 * n + 4 + 4 * c
    at = 4
    sids = np.frombuffer(raw, np.int64, m, at); at += 8 * m
    spx = np.frombuffer(raw, np.float32, 2 * m, at).reshape(m, 2); at += 8 * m
    found = np.frombuffer(raw, np.int32, n, at); at += 4 * n
    guess = np.frombuffer(raw, np.float32, 2 * n, at).reshape(n, 2); at += 8 * n
    n_guessed = struct.unpack_from("<i", raw, at)[0]; at += 4
    return dict(sids=sids, spx=spx, found=found, guess=guess, n_guessed=n_guessed, falls=np.frombuffer(raw, np.int32, c, at))


def check(driver, ids, cur, pred_ids, pred_px):
    """The program against the restatement, every output in every bit; returns the program's outputs."""
    o = host(driver, ids, cur, pred_ids, pred_px)
    w_guess, w_hit = fg.take_guess(cur, ids, pred_ids, pred_px)
    w_ids, w_px = fg.normalise(pred_ids, pred_px)
    assert np.array_equal(o["sids"], w_ids) and o["spx"].tobytes() == w_px.tobytes()
    assert np.array_equal(o["found"], fg.find(w_ids, ids)) and np.array_equal(o["found"] >= 0, w_hit)
    assert o["guess"].dtype == w_guess.dtype and o["guess"].tobytes() == w_guess.tobytes() and o["n_guessed"] == int(w_hit.sum())
    return o


def table(n, seed=1):
    """n rows with distinct ids in shuffled order, and their pixels."""
    rng = np.random.RandomState(seed)
    ids = (1000 + 3 * rng.permutation(n)).astype(np.int64)
    return ids, rng.uniform(0, 190, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("p", [0, 1, 2, 1024])
@pytest.mark.parametrize("n", [0, 1, 1024])
@pytest.mark.parametrize("hits", ["all", "none"])
def test_sizes_all_hit_and_none_hit(driver, n, p, hits):
    ids, cur = table(n)
    rng = np.random.RandomState(7 + p)
    if hits == "all":                                       # every listed id is a point's, as far as there are points
        pred_ids = (ids[rng.permutation(n)[:p]] if n else np.zeros(0, np.int64))
        pred_ids = np.concatenate([pred_ids, 10 ** 7 + np.arange(p - len(pred_ids))]).astype(np.int64)
    else:                                                   # ids between the table's: 1000 + 3 k + 1
        pred_ids = (1001 + 3 * rng.permutation(max(p, 1))[:p]).astype(np.int64)
    px = rng.uniform(0, 190, (p, 2)).astype(np.float32)
    o = check(driver, ids, cur, pred_ids, px)
    assert o["n_guessed"] == (min(n, p) if hits == "all" else 0)
    if o["n_guessed"] == 0:
        assert o["guess"].tobytes() == cur.tobytes()
    elif p >= n:
        assert not np.any(np.all(o["guess"] == cur, axis=1))


@pytest.mark.parametrize("where", ["table", "prediction", "both"])
def test_negative_ids_never_hit(driver, where):
    ids, cur = table(65)
    pred_ids, px = ids[::2].copy(), cur[::2] + np.float32(1.5)
    if where in ("table", "both"):
        ids[[0, 7, 64]] = -1
    if where in ("prediction", "both"):
        pred_ids = np.concatenate([[-1, -1], pred_ids, [-1]]).astype(np.int64)
        px = np.concatenate([[[5, 5], [6, 6]], px, [[7, 7]]]).astype(np.float32)
    o = check(driver, ids, cur, pred_ids, px)
    assert np.all(o["found"][ids < 0] == -1) and o["guess"][ids < 0].tobytes() == cur[ids < 0].tobytes()
    assert o["n_guessed"] == int(np.isin(ids[ids >= 0], pred_ids).sum()) > 20


def test_of_a_repeated_id_the_first_listed_row_counts(driver):
    ids, cur = table(9)
    pred_ids = np.array([ids[4], ids[2], ids[4], ids[4], ids[2]], np.int64)
    px = np.float32([[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]])
    o = check(driver, ids, cur, pred_ids, px)
    assert o["n_guessed"] == 2 and len(o["sids"]) == 2
    assert o["guess"][4].tolist() == [1, 2] and o["guess"][2].tolist() == [3, 4]


def test_descending_prediction_and_the_ends_of_int64(driver):
    ids = np.array([I64.max, 5, I64.min, 0, I64.max - 1, -1], np.int64)
    cur = np.arange(12, dtype=np.float32).reshape(6, 2)
    pred_ids = np.array([I64.max, I64.max - 1, 6, 5, 0, -1, I64.min], np.int64)         # descending
    px = 100 + np.arange(14, dtype=np.float32).reshape(7, 2)
    o = check(driver, ids, cur, pred_ids, px)
    assert np.all(np.diff(o["sids"]) > 0) and o["sids"][0] == I64.min and o["sids"][-1] == I64.max
    assert (o["found"] >= 0).tolist() == [True, True, False, True, True, False]           # INT64_MIN and -1 are listed and never match
    assert o["guess"][0].tolist() == [100, 101] and o["guess"][2].tolist() == [4, 5]


@pytest.mark.parametrize("min_tracked", [1, 10, 1024])
def test_fallback_at_its_boundary(driver, min_tracked):
    cases = [(1, min_tracked - 1, min_tracked), (1, min_tracked, min_tracked), (1, min_tracked + 1, min_tracked),
             (0, 0, min_tracked), (1, 0, 0), (0, 0, 0)]
    got = host(driver, [], np.zeros((0, 2)), [], np.zeros((0, 2)), cases)["falls"]
    assert got.tolist() == [int(fg.falls_back(*c)) for c in cases] == [1, 0, 0, 0, 0, 0]
