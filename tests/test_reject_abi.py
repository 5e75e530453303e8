"""The surface of the outlier rejection library (libvio_reject_hip.so): include/vio_reject.h compiles as C99 and C++11 on its own, the
library exports the vio_reject_ prefix, nothing else, and every function the header declares, and the constants of the header, the
binding and the restatement agree (the checks test_detect_abi.py makes for the detection library)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
HEADER, LIB, PREFIX = "vio_reject.h", "libvio_reject_hip.so", "vio_reject_"
BODY = ("vio_reject_item it; vio_reject_result o; vio_reject_config c; vio_reject_camera k; vio_reject_undistort_item u; "
        "(void)it; (void)o; (void)c; (void)k; (void)u; "
        "return VIO_REJECT_VERSION == 1 && VIO_REJECT_MAX_POINTS == 4096 && sizeof(vio_reject_result) == 88 && "
        "sizeof(vio_reject_config) == 24 && sizeof(vio_reject_camera) == 80 && sizeof(vio_reject_item) == 8 + 2 * sizeof(void *) && "
        "sizeof(vio_reject_undistort_item) == 16 + 6 * sizeof(void *) ? 0 : 1;")


def declared():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % PREFIX, txt)))


def header_values(name=HEADER, prefix="VIO_REJECT_"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return {k: v for k, v in re.findall(r"#define (%s[A-Z_]+) ([-0-9.e]+)" % prefix, txt)}


@pytest.mark.parametrize("cc,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_alone(tmp_path, cc, std, ext):
    if not shutil.which(cc):
        pytest.fail("%s not found" % cc)
    src = tmp_path / ("t." + ext)
    src.write_text('#include "%s"\nint main(void) { %s }\n' % (HEADER, BODY))
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])
    exe = tmp_path / "t"
    subprocess.check_call([cc, str(tmp_path / "t.o"), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_library_exports_its_prefix_only():
    lib = os.path.join(CSRC, LIB)
    assert os.path.exists(lib), "build first: %s" % lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    own = [ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-2] in ("T", "D", "B", "R", "W", "V")]
    assert own and all(s.startswith(PREFIX) for s in own), own
    names = declared()
    assert set(names) == {"vio_reject_create", "vio_reject_destroy", "vio_reject_last_error", "vio_reject_version", "vio_reject_set_camera",
                          "vio_reject_set_config", "vio_reject_batch", "vio_reject_undistort_batch", "vio_reject_lift",
                          "vio_reject_timing"}, names
    missing = [s for s in names if s not in own]
    assert not missing, missing


def test_restatement_constants_match_the_header():
    val = header_values()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import reject_reference as rr
    import sfm_reference as sr
    assert (int(val["VIO_REJECT_MAX_POINTS"]), int(val["VIO_REJECT_MAX_HYPOTHESES"]), int(val["VIO_REJECT_DEFAULT_HYPOTHESES"])) == \
        (rr.MAX_POINTS, rr.MAX_HYPOTHESES, rr.DEFAULT_HYPOTHESES) == (4096, 4096, 128)
    assert int(val["VIO_REJECT_MAX_ITEMS"]) == rr.MAX_ITEMS == 4096
    assert (float(val["VIO_REJECT_DEFAULT_F_THRESHOLD"]), float(val["VIO_REJECT_DEFAULT_FOCAL_LENGTH"])) == \
        (rr.DEFAULT_F_THRESHOLD, rr.DEFAULT_FOCAL_LENGTH) == (1.0, 460.0)
    assert (int(val["VIO_REJECT_LIFT_EVALUATIONS"]), int(val["VIO_REJECT_MIN_POINTS"])) == (rr.LIFT_EVALUATIONS, rr.MIN_POINTS) == (8, 8)
    assert (int(val["VIO_REJECT_ROUND"]), int(val["VIO_REJECT_THREADS"]), int(val["VIO_REJECT_ID_CHUNK"])) == (rr.ROUND, rr.THREADS, rr.ID_CHUNK)
    assert int(val["VIO_REJECT_FAIL_NO_MODEL"]) == rr.FAIL_NO_MODEL == 1
    # the round's 9 x 9 matrices fit a CU's LDS, and one more doubling would not
    assert 162 * 8 * rr.ROUND <= 160 * 1024 < 162 * 8 * 2 * rr.ROUND
    back = {k: v for k, v in re.findall(r"(VIO_[A-Z_]+)\s*=\s*(-?[0-9]+)", open(os.path.join(ROOT, "include", "vio_backend.h")).read())}
    assert int(back["VIO_OK"]) == rr.OK and int(back["VIO_ERR_NOT_FINITE"]) == rr.NOT_FINITE
    # the RANSAC is vio_sfm.h's, the point limit vio_detect.h's
    sfm = header_values("vio_sfm.h", "VIO_SFM_")
    assert int(val["VIO_REJECT_MAX_HYPOTHESES"]) == int(sfm["VIO_SFM_MAX_HYPOTHESES"])
    assert int(val["VIO_REJECT_DEFAULT_HYPOTHESES"]) == int(sfm["VIO_SFM_DEFAULT_HYPOTHESES"]) == sr.DEFAULT_CFG["ransac_hypotheses"]
    det = header_values("vio_detect.h", "VIO_DETECT_")
    assert int(val["VIO_REJECT_MAX_POINTS"]) == int(det["VIO_DETECT_MAX_POINTS"])
    # the restatement's camera is the reference configuration's
    assert (rr.EUROC["width"], rr.EUROC["height"], rr.EUROC["fx"], rr.EUROC["k1"]) == (752, 480, 461.6, -0.2917)


def test_python_binding_matches_the_header(vio):
    import ctypes as C
    from vio_amd import reject
    val = header_values()
    for k in ("MAX_POINTS", "MAX_ITEMS", "MAX_HYPOTHESES", "DEFAULT_HYPOTHESES", "LIFT_EVALUATIONS", "MIN_POINTS", "ROUND", "THREADS", "ID_CHUNK",
              "MODEL_PINHOLE", "FAIL_NO_MODEL"):
        assert getattr(reject, k) == int(val["VIO_REJECT_" + k]), k
    assert (reject.DEFAULT_F_THRESHOLD, reject.DEFAULT_FOCAL_LENGTH) == (float(val["VIO_REJECT_DEFAULT_F_THRESHOLD"]),
                                                                         float(val["VIO_REJECT_DEFAULT_FOCAL_LENGTH"]))
    assert C.sizeof(reject.VioRejectResult) == 88 and C.sizeof(reject.VioRejectConfig) == 24 and C.sizeof(reject.VioRejectCamera) == 80
    assert C.sizeof(reject.VioRejectItem) == 24 and C.sizeof(reject.VioRejectUndistortItem) == 64
    assert vio.REJECT_LIB.endswith(LIB) and vio.RejectHandle is reject.RejectHandle and vio.RejectLib is reject.RejectLib
    assert sorted(PREFIX + s for s in reject.RejectLib.SYMBOLS) == declared()


def test_handle_fails_with_a_status_without_a_gpu(vio):
    """On a machine without a GPU the create call returns a status (VioError), it does not crash; with one it succeeds."""
    lib = vio.load_reject()
    assert lib.fn["version"]() == 1
    try:
        h = lib.create()
    except vio.VioError as e:
        assert e.status in (-6, -2)
        return
    h.close()
