"""The join of vio_frame_read_batch (include/vio_frame_read.h) without a device.

1. csrc/vio_front_math.h (the rounding, the border test, the compaction's destination index, the id assignment) and the point
   bookkeeping of csrc/vio_frame_slots.h, compiled with tests/cpp/front_math_main.cpp into a stand-alone program (built as
   tests/test_frame_host_units.py builds its own; ASan and UBSan with VIO_TEST_SANITIZE=1; never loaded into Python).  Its output over
   scripted inputs equals a numpy restatement of the same glue, which is frontend.FeatureTracker's: in_border, the boolean reductions,
   update_ids, and prev_un stored before update_ids.
2. The surface: every new symbol is declared, exported and bound; the constants of the header, the binding and the two csrc headers agree;
   the header compiles alone as C99 and C++11.
3. frontend.BatchFeatureTracker over a stand-in handle: what it configures, what it passes on, and feature_frames().
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
OK, BAD_SLOT, TWICE, BAD_DIMS, SMALL_LEVEL, GEOMETRY, TOO_FEW, MASK_GEOMETRY, BAD_TIME, BAD_POINTS = range(10)
CAP = 1024
NEW = ["set_camera", "set_tracker", "read_batch", "points_set", "points_get", "read_timing"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("front_math")
    exe = d / "front_math"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if os.environ.get("VIO_TEST_SANITIZE") == "1" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "front_math_main.cpp")])
    return d, str(exe)


def run(driver, script):
    d, exe = driver
    fin, fout = str(d / "in.txt"), str(d / "out.txt")
    open(fin, "w").write("\n".join(script) + "\n")
    subprocess.check_call([exe, fin, fout])
    lines = [ln.split() for ln in open(fout).read().splitlines()]
    assert len(lines) == len(script)
    return lines


def in_border(pts, w, h, b):
    """frontend.FeatureTracker.in_border."""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(pts, dtype=np.float64).reshape(-1, 2))
    return (b <= r[:, 0]) & (r[:, 0] < w - b) & (b <= r[:, 1]) & (r[:, 1] < h - b)


def k_line(b, w, h, pts, status):
    return "K %d %d %d %d " % (b, w, h, len(pts)) + " ".join("%.9g %.9g %d" % (x, y, s) for (x, y), s in zip(pts.tolist(), status.tolist()))


def check_k(line, b, w, h, pts, status):
    keep = (status == 0) & in_border(pts, w, h, b)
    v = [int(x) for x in line[1:]]
    assert line[0] == "K" and v[0] == int(keep.sum())
    got_keep, got_dest = np.array(v[1::2], dtype=bool), np.array(v[2::2])
    assert np.array_equal(got_keep, keep), (b, w, h, pts[got_keep != keep])
    # a stable compaction: a[keep] of numpy
    assert np.array_equal(got_dest[keep], np.arange(keep.sum())) and np.all(got_dest[~keep] == -1)
    return keep


def test_rounding_and_border(driver):
    """Ties to even at x.5, the border at b and at w - b - 0.5, what is not a number."""
    cases = []
    for b, w, h in [(1, 64, 48), (2, 65, 17), (0, 33, 9), (8, 64, 48)]:
        xs = [b - 1.0, b - 0.5, b - 0.4999, b, b + 0.5, w - b - 1.5, w - b - 1.0, w - b - 0.5, w - b - 0.4999, w - b, 0.5, 1.5, 2.5, 3.5, -0.5, -0.0]
        pts = np.float32([[x, h / 2.0] for x in xs] + [[w / 2.0, y] for y in [b - 0.5, b, h - b - 0.5, h - b - 1.0, h - b]] +
                         [[np.nan, 3.0], [3.0, np.nan], [np.inf, 3.0], [-np.inf, 3.0], [3.0e9, 3.0], [-3.0e9, 3.0]])
        status = np.zeros(len(pts), dtype=np.int64)
        cases.append((b, w, h, pts, status))
    lines = run(driver, [k_line(*c) for c in cases])
    seen = set()
    for c, ln in zip(cases, lines):
        keep = check_k(ln, *c)
        b, w, h, pts, _ = c
        seen |= {(float(x) % 1.0 == 0.5, bool(k)) for (x, _), k in zip(pts.tolist(), keep.tolist()) if np.isfinite(x)}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}                 # ties went both ways
    # the two the issue names, spelled out: 0.5 rounds to 0, outside b = 1; 62.5 rounds to 62, inside 64 - 1; 63.5 rounds to 64, outside 65 - 1
    assert not in_border(np.float32([[0.5, 5]]), 64, 48, 1)[0] and in_border(np.float32([[62.5, 5]]), 64, 48, 1)[0]
    assert not in_border(np.float32([[63.5, 5]]), 65, 48, 1)[0] and in_border(np.float32([[1.5, 5]]), 65, 48, 2)[0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200, 1023, 1024])
def test_compaction_order(driver, n):
    """Rows across wavefront boundaries, lost ones and ones outside the border mixed: the kept rows keep their order."""
    rng = np.random.RandomState(n)
    pts = np.stack([rng.uniform(-2, 66, n), rng.uniform(-2, 50, n)], axis=1).astype(np.float32)
    status = (rng.uniform(size=n) < 0.3).astype(np.int64) * rng.choice([1, 2, -3], size=n)
    cases = [(1, 64, 48, pts, status), (1, 64, 48, pts, np.zeros(n, dtype=np.int64)), (1, 64, 48, pts, np.ones(n, dtype=np.int64))]
    for c, ln in zip(cases, run(driver, [k_line(*c) for c in cases])):
        check_k(ln, *c)


def test_id_assignment_and_the_prev_un_quirk(driver):
    """A sequence of frames through the program's counter against frontend.FeatureTracker's order of operations: prev_un takes the ids
    before update_ids, update_ids numbers the rows without an id in row order."""
    rng = np.random.RandomState(4)
    frames, ids, n_id = [], np.zeros(0, dtype=np.int64), 0
    want = []
    for t in range(6):
        keep = rng.uniform(size=len(ids)) < 0.7
        n_new = [70, 0, 130, 5, 0, 1024][t]
        ids = np.concatenate([ids[keep], np.full(n_new, -1, dtype=np.int64)])[:CAP]
        if t == 3:
            ids = rng.permutation(ids)                                   # (setMask reorders: old and new rows interleave)
        frames.append(ids.copy())
        prev_un = ids.copy()                                             # undistortedPoints runs before updateID
        new = np.nonzero(ids == -1)[0]                                   # FeatureTracker.update_ids
        ids[new] = n_id + np.arange(len(new))
        n_id += len(new)
        want.append((n_id, prev_un, ids.copy()))
    lines = run(driver, ["U %d " % len(f) + " ".join(str(int(i)) for i in f) for f in frames])
    for (n_id, prev_un, ids), ln in zip(want, lines):
        v = [int(x) for x in ln[1:]]
        assert ln[0] == "U" and v[0] == n_id
        assert np.array_equal(v[1::2], prev_un) and np.array_equal(v[2::2], ids)
    assert any(np.any(p == -1) for _, p, _ in want) and len(set(want[-1][2].tolist())) == len(want[-1][2])


def table(line):
    """(letter, code, bad, {slot: (n_frames, n_pts, n_prev_un, next_id, n_read, time)})"""
    rest, slots = line[3:], {}
    while rest:
        assert rest[0] == "slot"
        slots[int(rest[1])] = tuple(int(x) for x in rest[2:7]) + (float(rest[7]),)
        rest = rest[8:]
    return line[0], int(line[1]), int(line[2]), slots


def test_point_bookkeeping(driver):
    """The slot table's mirror of the resident points over a scripted sequence, against a model written out here."""
    A, B = (64, 48), (40, 24)
    ops = [
        ("S", 0, 5, TOO_FEW),                                               # no frame to lie in
        ("E", 1, [(0,) + A + (0.0, 24, 24)], OK),
        ("E", 1, [(0,) + A + (0.05, 20, 30)], OK),
        ("E", 1, [(0,) + A + (0.05, 20, 30)], BAD_TIME),                    # a time that does not increase
        ("E", 0, [(1,) + B + (0.0, 0, 0), (0,) + A + (0.01, 1, 1)], BAD_TIME),      # ... in a later item: slot 1 stays empty
        ("E", 1, [(0,) + A + (float("nan"), 1, 1)], BAD_TIME),
        ("E", 1, [(0,) + B + (0.1, 1, 1)], GEOMETRY),
        ("E", 1, [(0,) + A + (0.1, 1, 1), (0,) + A + (0.1, 1, 1)], TWICE),
        ("P", 0) + A + (OK,),                                               # a direct push drops the points, nothing else
        ("E", 0, [(0,) + A + (0.1, 0, 30)], OK),
        ("S", 0, 9, OK), ("S", 0, 1025, BAD_POINTS), ("S", 0, -1, BAD_POINTS), ("S", 256, 1, BAD_SLOT),
        ("E", 1, [(0,) + A + (0.15, 9, 31), (1,) + B + (7.0, 3, 3)], OK),
        ("M", 1, 32, 24, OK),
        ("E", 1, [(1,) + B + (8.0, 3, 3)], MASK_GEOMETRY),                  # with publish the mask must fit ...
        ("E", 0, [(1,) + B + (8.0, 2, 3)], OK),                             # ... without, nothing reads it
        ("R", 0, OK),                                                       # the counter stays, the rest goes
        ("E", 1, [(0,) + B + (-5.0, 4, 35)], OK),                           # another geometry, an earlier time: a new stream
        ("L", 2, OK),                                                       # other levels: every slot is reset
        ("E", 1, [(1,) + B + (0.0, 2, 5)], MASK_GEOMETRY), ("C", 1, OK), ("E", 1, [(1,) + B + (0.0, 2, 5)], OK),
    ]
    script = []
    for op in ops:
        if op[0] == "E":
            script.append("E %d %d " % (op[1], len(op[2])) + " ".join("%d %d %d %r %d %d" % it for it in op[2]))
        else:
            script.append(" ".join(str(x) for x in op[:-1]))
    model = {}                                                              # slot -> [n_frames, n_pts, n_prev_un, next_id, n_read, time]
    for op, ln in zip(ops, run(driver, script)):
        letter, code, bad, tab = table(ln)
        assert letter == op[0] and code == op[-1], (op, ln)
        if op[0] == "E" and code == OK:
            for (s, w, h, time, rows, nid) in op[2]:
                m = model.setdefault(s, [0, 0, 0, 0, 0, 0.0])
                model[s] = [min(m[0] + 1, 2), rows, rows, nid, m[4] + 1, time]
        elif op[0] == "E":
            want_bad = {BAD_TIME: lambda: next(i for i, it in enumerate(op[2]) if not (np.isfinite(it[3]) and (model.get(it[0], [0] * 6)[2] == 0 or it[3] > model[it[0]][5]))),
                        GEOMETRY: lambda: 0, TWICE: lambda: 1, MASK_GEOMETRY: lambda: 0}[code]()
            assert bad == want_bad, (op, ln)
        elif op[0] == "P" and code == OK:
            m = model[op[1]]
            m[0], m[1] = min(m[0] + 1, 2), 0
        elif op[0] == "S" and code == OK:
            model[op[1]][1] = op[2]
        elif op[0] == "R":
            model[op[1]] = [0, 0, 0, model[op[1]][3], 0, 0.0]
        elif op[0] == "L":
            model = {s: [0, 0, 0, m[3], 0, 0.0] for s, m in model.items()}
        want = {s: tuple(m) for s, m in model.items() if any(m[:5])}
        assert tab == want, (op, tab, want)
    assert model[0][3] == 35 and model[1] == [1, 2, 2, 5, 1, 0.0]


# ---- the surface ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(vio):
    from vio_amd import frame
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vio_frame_read.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(vio_frame_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted("vio_frame_" + s for s in NEW)
    lib = os.path.join(CSRC, "libvio_frame_hip.so")
    assert os.path.exists(lib), "build first: %s" % lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    own = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert all(s in own for s in declared), sorted(set(declared) - own)
    assert frame.FrameLib.READ_SYMBOLS == NEW
    fn = vio.load_frame().fn
    assert all(fn[s] is not None for s in NEW) and fn["version"]() == 1       # the addition is advertised by VIO_FRAME_HAS_READ, not a version
    assert '#include "vio_frame_read.h"' in open(os.path.join(ROOT, "include", "vio_frame.h")).read()
    for m in ("set_camera", "set_tracker", "read_batch", "points_set", "points_get", "read_timing"):
        assert callable(getattr(frame.FrameHandle, m)), m
    assert vio.BatchFeatureTracker is vio.frontend.BatchFeatureTracker


def test_constants_and_struct_sizes_agree(vio):
    from vio_amd import frame
    hdr = open(os.path.join(ROOT, "include", "vio_frame_read.h")).read()
    val = dict(re.findall(r"#define (VIO_FRAME_[A-Z_]+) ([0-9]+)", hdr + open(os.path.join(ROOT, "include", "vio_frame.h")).read()))
    assert val["VIO_FRAME_HAS_READ"] == "1" and val["VIO_FRAME_VERSION"] == "1"
    cap = int(val["VIO_FRAME_MAX_TRACK_POINTS"])
    assert cap == CAP == frame.MAX_TRACK_POINTS
    assert (frame.DEFAULT_MAX_CNT, frame.DEFAULT_TRACK_BORDER) == (int(val["VIO_FRAME_DEFAULT_MAX_CNT"]), int(val["VIO_FRAME_DEFAULT_BORDER"])) == (150, 1)
    slots = open(os.path.join(CSRC, "vio_frame_slots.h")).read()
    math = open(os.path.join(CSRC, "vio_front_math.h")).read()
    assert int(re.search(r"constexpr int FRAME_MAX_TRACK_POINTS = ([0-9]+);", slots).group(1)) == cap
    assert int(re.search(r"constexpr int FRONT_CAP = ([0-9]+);", math).group(1)) == cap
    for other, family in (("vio_detect.h", "DETECT"), ("vio_reject.h", "REJECT"), ("vio_flow.h", "FLOW")):
        most = re.search(r"#define VIO_%s_MAX_POINTS ([0-9]+)" % family, open(os.path.join(ROOT, "include", other)).read())
        assert cap <= int(most.group(1)), other
    assert C.sizeof(frame.VioFrameReadItem) == 72 and C.sizeof(frame.VioFrameReadResult) == 40
    # plain C++ a host build can include
    for src in (slots, math):
        assert "hip_runtime" not in src


@pytest.mark.parametrize("cc,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_alone(tmp_path, cc, std, ext):
    if not shutil.which(cc):
        pytest.fail("%s not found" % cc)
    body = ("vio_frame_read_item i; vio_frame_read_result r; (void)i; (void)r; return VIO_FRAME_HAS_READ == 1 && VIO_FRAME_MAX_TRACK_POINTS == 1024 && "
            "sizeof(vio_frame_read_item) == 24 + 6 * sizeof(void *) && sizeof(vio_frame_read_result) == 40 ? 0 : 1;")
    for header in ("vio_frame_read.h", "vio_frame.h"):
        src = tmp_path / ("t_%s.%s" % (header[:-2], ext))
        src.write_text('#include "%s"\nint main(void) { %s }\n' % (header, body))
        exe = tmp_path / ("t_" + header[:-2])
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        assert subprocess.call([str(exe)]) == 0


# ---- BatchFeatureTracker over a stand-in ----------------------------------------------------------------------
class StandIn:
    def __init__(self):
        self.calls = []

    def set_config(self, **k):
        self.calls.append(("set_config", k))

    def set_tracker(self, **k):
        self.calls.append(("set_tracker", k))

    def set_mask(self, mask, slot=0):
        self.calls.append(("set_mask", slot))

    def read_batch(self, imgs, times, slots=None, publish=True):
        self.calls.append(("read_batch", times, list(slots), publish))
        out = []
        for s in slots:
            n = 3 + s
            out.append(dict(pts=np.arange(2 * n, dtype=np.float32).reshape(n, 2), ids=np.arange(n, dtype=np.int64) + 10 * s,
                            track_cnt=(np.arange(n, dtype=np.int32) % 3), un_pts=np.full((n, 2), 0.5, np.float32),
                            velocity=np.full((n, 2), -2.0, np.float32), n=n, n_new=1))
        return out


def test_batch_feature_tracker_over_a_stand_in(vio):
    st = StandIn()
    mask = np.full((4, 4), 255, np.uint8)
    bt = vio.BatchFeatureTracker(st, slots=[2, 0], max_cnt=40, min_dist=3, border=2, masks={0: mask})
    assert st.calls == [("set_config", dict(detect=dict(min_distance=3))), ("set_tracker", dict(max_cnt=40, border=2)), ("set_mask", 0)]
    with pytest.raises(RuntimeError):
        bt.feature_frames()
    img = np.zeros((4, 4), np.uint8)
    outs = bt.read_images([img, img], 0.25, publish=False)
    assert st.calls[-1] == ("read_batch", 0.25, [2, 0], False) and [o["n"] for o in outs] == [5, 3]
    for (ids, rows), o in zip(bt.feature_frames(), outs):
        k = o["track_cnt"] > 1                                       # what FeatureTracker.feature_frame publishes
        assert ids.dtype == np.int64 and rows.dtype == np.float64 and rows.shape == (int(k.sum()), 7)
        assert np.array_equal(ids, o["ids"][k]) and np.array_equal(rows[:, 3:5], o["pts"][k])
        assert np.all(rows[:, 0:2] == 0.5) and np.all(rows[:, 2] == 1.0) and np.all(rows[:, 5:7] == -2.0)
    with pytest.raises(ValueError):
        bt.read_images([img], 0.5)
    with pytest.raises(ValueError):
        bt.read_images([img, img.astype(np.float32)], 0.5)
    with pytest.raises(ValueError):
        vio.BatchFeatureTracker(st, slots=[1, 1])
