"""The surface of the non-keyframe PnP library (libvio_pnp_hip.so): include/vio_pnp.h compiles as C99 and C++11 on its own, the library
exports the vio_pnp_ prefix, nothing else, and every function the header declares, and the restatement's constants are the header's
(the checks test_sfm_abi.py makes for the SfM library)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
HEADER, LIB, PREFIX = "vio_pnp.h", "libvio_pnp_hip.so", "vio_pnp_"
BODY = ("vio_pnp_item it; vio_pnp_result r; vio_pnp_frame_info o; vio_pnp_config c; (void)it; (void)r; (void)o; (void)c; "
        "return VIO_PNP_VERSION == 1 && VIO_PNP_MAX_FRAMES == 32 && VIO_SFM_PNP_MAX_ITER == 20 ? 0 : 1;")


def declared():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % PREFIX, txt)))


@pytest.mark.parametrize("cc,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_alone(tmp_path, cc, std, ext):
    if not shutil.which(cc):
        pytest.fail("%s not found" % cc)
    src = tmp_path / ("t." + ext)
    src.write_text('#include "%s"\nint main(void) { %s }\n' % (HEADER, BODY))
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_library_exports_its_prefix_only():
    lib = os.path.join(CSRC, LIB)
    assert os.path.exists(lib), "build first: %s" % lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    own = [ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-2] in ("T", "D", "B", "R", "W", "V")]
    assert own and all(s.startswith(PREFIX) for s in own), own
    names = declared()
    assert set(names) >= {"vio_pnp_create", "vio_pnp_destroy", "vio_pnp_last_error", "vio_pnp_version", "vio_pnp_set_config",
                          "vio_pnp_frames_batch", "vio_pnp_timing"}, names
    missing = [s for s in names if s not in own]
    assert not missing, missing


def test_binding_constants_match_the_header():
    import sys
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    val = {k: v for k, v in re.findall(r"#define (VIO_PNP_[A-Z_]+) ([-0-9.e]+)", txt)}
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pnp_reference as pr
    assert int(val["VIO_PNP_DEFAULT_MIN_POINTS"]) == pr.MIN_POINTS == pr.DEFAULT_CFG["min_points"]
    assert int(val["VIO_PNP_MAX_FRAMES"]) == pr.MAX_FRAMES and int(val["VIO_PNP_MAX_POINTS"]) == pr.MAX_POINTS
    assert (int(val["VIO_PNP_FAIL_FEW_POINTS"]), int(val["VIO_PNP_FAIL_NO_POSE"])) == (pr.FAIL_FEW_POINTS, pr.FAIL_NO_POSE)
    back = {k: v for k, v in re.findall(r"(VIO_[A-Z_]+)\s*=\s*(-?[0-9]+)", open(os.path.join(ROOT, "include", "vio_backend.h")).read())}
    assert int(back["VIO_OK"]) == pr.OK and int(back["VIO_ERR_NOT_FINITE"]) == pr.NOT_FINITE


def test_python_binding_matches_the_header(vio):
    import sys
    from vio_amd import pnp
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pnp_reference as pr
    assert (pnp.MAX_FRAMES, pnp.MAX_POINTS, pnp.DEFAULT_MIN_POINTS) == (pr.MAX_FRAMES, pr.MAX_POINTS, pr.MIN_POINTS)
    assert (pnp.OK, pnp.NOT_FINITE, pnp.FAIL_FEW_POINTS, pnp.FAIL_NO_POSE) == (pr.OK, pr.NOT_FINITE, pr.FAIL_FEW_POINTS, pr.FAIL_NO_POSE)


def test_handle_fails_with_a_status_without_a_gpu(vio):
    """On a machine without a GPU the create call returns a status (VioError), it does not crash; with one it succeeds."""
    lib = vio.load_pnp()
    assert lib.fn["version"]() == 1
    try:
        h = lib.create()
    except vio.VioError as e:
        assert e.status in (-6, -2)
        return
    h.close()
