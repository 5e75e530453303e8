"""The host sides of the four front-end stages (csrc/vio_{clahe,flow,detect,reject}_host.h), which the stand-alone libraries and
libvio_frame_hip both include, compiled by g++ with tests/cpp/front_host_main.cpp into a stand-alone program, with no HIP header: the
config checks, the tracked-point check, the table sizes, the flow levels and the unpacking of the detection results.  Every error text
here is a literal copied from the sources as they were while each library still had its own copy of the check, so a shared helper that
changed a byte of one would fail.  With VIO_TEST_SANITIZE=1 it is built with ASan and UBSan.  It is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("front_host")
    exe = d / "front_host"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if os.environ.get("VIO_TEST_SANITIZE") == "1" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "front_host_main.cpp")])
    return d, str(exe)


def run(driver, script):
    """[(fields before the first '|', [the texts behind each '|'])] per line of the script"""
    d, exe = driver
    fin, fout = str(d / "in.txt"), str(d / "out.txt")
    open(fin, "w").write("\n".join(script) + "\n")
    subprocess.check_call([exe, fin, fout])
    lines = open(fout).read().splitlines()
    assert len(lines) == len(script)
    out = []
    for ln in lines:
        parts = ln.split("|")
        out.append((parts[0].split(), parts[1:]))
    return out


CLAHE_TEXT = "%s: clip_limit finite and >= 0, tiles_x and tiles_y in [1, 16]"
FLOW_TEXT = "%s: levels in [1, 8], half_patch in [1, 16], max_iter in [1, 1000], inverse and early_stop 0 or 1, border >= 0"
DETECT_TEXT = "%s: quality in (0, 1], min_distance >= 0"
REJECT_TEXT = "%s: ransac_hypotheses in [1, 4096], f_threshold and focal_length finite and > 0"


def test_defaults_pass(driver):
    (f, t), = run(driver, ["DF"])
    assert f == ["OK"] * 4 and t == [""]


def check_config(driver, cmd, names, text, good, bad):
    """every row of good passes and leaves no text; every row of bad fails with the text, under each of the two function names"""
    for fn in names:
        rows = run(driver, ["%s %s %s" % (cmd, fn, r) for r in good + bad])
        for r, (f, t) in zip(good + bad, rows):
            if r in good:
                assert f == ["OK"] and t == [""], (fn, r, f, t)
            else:
                assert f == ["BAD_ARG"] and t == [text % fn], (fn, r, f, t)


def test_clahe_config(driver):
    good = ["3.0 8 8", "0 1 1", "1e300 16 16", "0.5 1 16"]
    bad = ["-1e-9 8 8", "nan 8 8", "inf 8 8", "-inf 8 8", "3 0 8", "3 17 8", "3 8 0", "3 8 17"]
    check_config(driver, "CC", ["vio_clahe_set_config", "vio_frame_set_config"], CLAHE_TEXT, good, bad)


def test_flow_config(driver):
    good = ["4 4 10 0 1 0", "1 1 1 0 0 0", "8 16 1000 1 0 1", "4 4 10 1 1000000 1"]
    bad = ["0 4 10 0 1 0", "9 4 10 0 1 0", "4 0 10 0 1 0", "4 17 10 0 1 0", "4 4 0 0 1 0", "4 4 1001 0 1 0", "4 4 10 -1 1 0", "4 4 10 2 1 0",
           "4 4 10 0 -1 0", "4 4 10 0 1 -1", "4 4 10 0 1 2"]
    check_config(driver, "CF", ["vio_flow_set_config", "vio_frame_set_config"], FLOW_TEXT, good, bad)


def test_detect_config(driver):
    good = ["0.01 30", "1 0", "1e-300 1000000"]
    bad = ["0 30", "-0.01 30", "1.0000000000000002 30", "nan 30", "inf 30", "-inf 30", "0.01 -1"]
    check_config(driver, "CD", ["vio_detect_set_config", "vio_frame_set_config"], DETECT_TEXT, good, bad)


def test_reject_config(driver):
    good = ["128 1.0 460.0", "1 1e-300 1e-300", "4096 1e300 1e300"]
    bad = ["0 1 460", "4097 1 460", "128 0 460", "128 -1 460", "128 nan 460", "128 inf 460", "128 1 0", "128 1 -460", "128 1 nan", "128 1 inf"]
    check_config(driver, "CR", ["vio_reject_set_config", "vio_frame_set_camera"], REJECT_TEXT, good, bad)


def test_reject_camera(driver):
    ok = "0 460 460 376 240 0 0 0 0 752 480"
    for fn in ["vio_reject_set_camera", "vio_frame_set_camera"]:
        cases = [(ok, None), ("0 -460 1e-300 0 0 -0.3 0.1 1e-3 -1e-3 1 1", None),
                 ("1 460 460 376 240 0 0 0 0 752 480", "%s: model 1: only PINHOLE is built"),
                 ("-1 460 460 376 240 0 0 0 0 752 480", "%s: model -1: only PINHOLE is built"),
                 ("0 0 460 376 240 0 0 0 0 752 480", "%s: fx, fy must not be 0, width and height at least 1"),
                 ("0 460 0 376 240 0 0 0 0 752 480", "%s: fx, fy must not be 0, width and height at least 1"),
                 ("0 460 460 376 240 0 0 0 0 0 480", "%s: fx, fy must not be 0, width and height at least 1"),
                 ("0 460 460 376 240 0 0 0 0 752 0", "%s: fx, fy must not be 0, width and height at least 1"),
                 # the model is looked at first, a value that is not finite before the zeros
                 ("2 nan 0 376 240 0 0 0 0 0 0", "%s: model 2: only PINHOLE is built"),
                 ("0 0 460 376 240 0 0 0 inf 0 480", "%s: a parameter is not finite")]
        cases += [("0 " + " ".join(bad if k == j else v for j, v in enumerate("460 460 376 240 0 0 0 0".split())) + " 752 480",
                   "%s: a parameter is not finite") for k in range(8) for bad in ("nan", "inf", "-inf")]
        rows = run(driver, ["CM %s %s" % (fn, c) for c, _ in cases])
        for (c, text), (f, t) in zip(cases, rows):
            assert (f, t) == ((["OK"], [""]) if text is None else (["BAD_ARG"], [text % fn])), (fn, c, f, t)


def test_detect_counts(driver):
    text = "item 7: n_tracked and max_total must be in [0, 4096]"
    for fn, pre in [("-", ""), ("vio_frame_detect_batch", "vio_frame_detect_batch: ")]:
        good, bad = ["0 0", "4096 4096", "1 0", "0 1"], ["-1 0", "4097 0", "0 -1", "0 4097"]
        rows = run(driver, ["N %s %s" % (fn, r) for r in good + bad])
        for r, (f, t) in zip(good + bad, rows):
            assert (f, t) == ((["OK"], [""]) if r in good else (["BAD_ARG"], [pre + text])), (fn, r, f, t)


def test_tracked_points_on_a_3_by_2_image(driver):
    """rx = nearbyint(x) must be in [0, 3), ry = nearbyint(y) in [0, 2): halves round to even, and -0.5 rounds to -0, which is not < 0."""
    out = "item 7: tracked point %d (%s) rounds to a pixel outside the 3 x 2 image"
    cases = [
        ("0", "OK", 1, None),
        ("1 -0.5 -0.5", "OK", 1, None), ("1 0.5 0.5", "OK", 1, None), ("2 0 0 2 1", "OK", 1, None),
        ("1 2.5 0", "OK", 1, None),                                     # 2.5 rounds to 2
        ("1 3.0 0", "BAD_ARG", 1, (0, "3, 0")),
        ("1 2.5000002 0", "BAD_ARG", 1, (0, "2.5, 0")),                    # the next float above 2.5 rounds to 3; %g prints six digits
        ("1 0 1.5", "BAD_ARG", 1, (0, "0, 1.5")),                          # 1.5 rounds to 2
        ("1 0 2.0", "BAD_ARG", 1, (0, "0, 2")),
        ("1 0 1.4999999", "OK", 1, None),
        ("1 -0.50000006 0", "BAD_ARG", 1, (0, "-0.5, 0")),
        ("2 1 1 -1 0", "BAD_ARG", 1, (1, "-1, 0")),                        # the message names the point
        # a point that is not finite makes the item inactive and is no error; the points behind it are still checked
        ("1 nan 0", "OK", 0, None), ("1 0 nan", "OK", 0, None), ("1 inf 0", "OK", 0, None), ("1 0 -inf", "OK", 0, None),
        ("3 1 1 nan nan 2 1", "OK", 0, None), ("3 1 1 nan 0 3 1", "BAD_ARG", 0, (2, "3, 1")),
    ]
    for fn, pre in [("-", ""), ("vio_frame_detect_batch", "vio_frame_detect_batch: ")]:
        rows = run(driver, ["T %s %s" % (fn, c[0]) for c in cases])
        for (c, status, active, msg), (f, t) in zip(cases, rows):
            assert f == [status, str(active)], (fn, c, f, t)
            assert t == ([""] if msg is None else [pre + out % msg]), (fn, c, f, t)


def align256(x):
    return (x + 255) // 256 * 256


def test_detect_table_sizes(driver):
    """The three buffers of a detection call, as vio_detect_batch and vio_frame_detect_batch carved them before they shared det_sizes:
    uploaded DetItemD[count] | DetTrk[n_trk]; read back DetRes[count] | keep_order[n_trk] | new_pts[n_new][2]; scratch tkey[n_trk] |
    kept_xy[n_trk][2]."""
    ITEM, TRK, RES = 80, 16, 24        # 8 int32 + 2 addresses + 2 int64 + 4 int32; 4 int32; 4 int32 + 1 uint64
    cases = [(c, t, n) for c in (0, 1, 4096) for t in (0, 1) for n in (0, 1)] + [(4096, 4096 * 4096, 4096 * 4096), (3, 17, 5)]
    rows = run(driver, ["S %d %d %d" % c for c in cases])
    for (count, n_trk, n_new), (f, _) in zip(cases, rows):
        b_it, b_tab, b_res, b_keep, b_out, b_key, b_scratch, s_item, s_trk, s_res = [int(x) for x in f]
        assert (s_item, s_trk, s_res) == (ITEM, TRK, RES)
        # the parent's formulas
        assert b_it == align256(ITEM * count) and b_tab == b_it + TRK * n_trk
        assert b_res == align256(RES * count) and b_keep == align256(4 * n_trk) and b_out == b_res + b_keep + 4 * 2 * n_new
        assert b_key == align256(8 * n_trk) and b_scratch == b_key + 4 * 2 * n_trk
        # every part starts on a 256-byte boundary and ends before the next starts
        tab = [(0, ITEM * count), (b_it, TRK * n_trk)]
        out = [(0, RES * count), (b_res, 4 * n_trk), (b_res + b_keep, 8 * n_new)]
        scratch = [(0, 8 * n_trk), (b_key, 8 * n_trk)]
        for parts, total in ((tab, b_tab), (out, b_out), (scratch, b_scratch)):
            assert all(at % 256 == 0 for at, _ in parts)
            ends = [at + size for at, size in parts]
            assert all(e <= nxt for e, nxt in zip(ends, [at for at, _ in parts][1:] + [total])) and ends[-1] == total


def test_flow_levels(driver):
    rows = run(driver, ["L 4 4 2", "L 4 4 3", "L 5 4 2", "L 752 480 4", "L 2 2 1", "L 1 2 1", "L 16384 16384 8"])
    assert rows[1][0] == ["0"] and rows[5][0] == ["0"]
    want = {0: [(4, 4), (2, 2)], 2: [(5, 4), (2, 2)], 3: [(752, 480), (376, 240), (188, 120), (94, 60)], 4: [(2, 2)],
            6: [(16384 >> l, 16384 >> l) for l in range(8)]}
    for k, levels in want.items():
        f = [int(x) for x in rows[k][0]]
        assert f[:3] == [1, 1, 1] and len(f) == 3 + 5 * len(levels), (k, f)
        for l, (w, h) in enumerate(levels):
            # the descriptor's w, h and (rows tightly packed) pitch, and frame_layout's w and h
            assert f[3 + 5 * l:8 + 5 * l] == [w, h, w, w, h], (k, l, f)


def test_detect_unpack_clamps_and_stays_inside(driver):
    """The device's counts are bounded by what the caller's arrays hold; the item's rows start at 2 (keep_order: 102, 103, ...) and 3
    (new_pts: 1006, ...) of the call's tables."""
    cases = [
        ("3 2 1 -1 -1", "OK OK 0 0", [-1, -1, -1], -1.0),
        ("3 2 1 4 3", "OK OK 3 2", [102, 103, 104], 1006.0),
        ("3 2 1 2 1", "OK OK 2 1", [102, 103, -1], 1006.0),
        ("3 2 1 2147483647 -2147483648", "OK OK 3 0", [102, 103, 104], -1.0),
        ("0 0 1 1 1", "OK OK 0 0", [], -1.0),
        ("1 0 1 5 5", "OK OK 1 0", [102], -1.0),
        ("0 1 1 5 5", "OK OK 0 1", [], 1006.0),
        ("3 2 0 3 2", "NOT_FINITE NOT_FINITE 0 0", [-1, -1, -1], -1.0),
    ]
    rows = run(driver, ["U " + c[0] for c in cases])
    for (c, head, keep, first_new), (f, t) in zip(cases, rows):
        assert f[:4] == head.split(), (c, f, t)
        active = head.startswith("OK")
        assert (int(f[4]), float(f[5])) == ((11, 2.5) if active else (0, 0.0)), (c, f)
        assert f[6] == "1", "a write landed outside the caller's arrays: %r" % (c,)
        assert float(f[7]) == first_new and [int(x) for x in t[0].split()] == keep, (c, f, t)
        assert t[1] == ("" if active else "item 0: a tracked point is not finite")
