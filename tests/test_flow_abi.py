"""The surface of the feature tracking library (libvio_flow_hip.so): include/vio_flow.h compiles as C99 and C++11 on its own, the
library exports the vio_flow_ prefix, nothing else, and every function the header declares, and the constants of the header, the
binding and the restatement agree (the checks test_pnp_abi.py makes for the PnP library)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
HEADER, LIB, PREFIX = "vio_flow.h", "libvio_flow_hip.so", "vio_flow_"
BODY = ("vio_flow_item it; vio_flow_pt_info o; vio_flow_config c; (void)it; (void)o; (void)c; "
        "return VIO_FLOW_VERSION == 1 && VIO_FLOW_MAX_LEVELS == 8 && sizeof(vio_flow_pt_info) == 16 ? 0 : 1;")


def declared():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % PREFIX, txt)))


def header_values():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    return {k: v for k, v in re.findall(r"#define (VIO_FLOW_[A-Z_]+) ([-0-9.e]+)", txt)}


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
    assert set(names) >= {"vio_flow_create", "vio_flow_destroy", "vio_flow_last_error", "vio_flow_version", "vio_flow_set_config",
                          "vio_flow_track_batch", "vio_flow_pyramid", "vio_flow_timing"}, names
    missing = [s for s in names if s not in own]
    assert not missing, missing


def test_restatement_constants_match_the_header():
    val = header_values()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import flow_reference as fr
    assert (int(val["VIO_FLOW_MAX_LEVELS"]), int(val["VIO_FLOW_MAX_HALF_PATCH"]), int(val["VIO_FLOW_MAX_POINTS"])) == \
        (fr.MAX_LEVELS, fr.MAX_HALF_PATCH, fr.MAX_POINTS)
    cfg = fr.DEFAULT_CFG
    assert (int(val["VIO_FLOW_DEFAULT_LEVELS"]), int(val["VIO_FLOW_DEFAULT_HALF_PATCH"]), int(val["VIO_FLOW_DEFAULT_MAX_ITER"]),
            int(val["VIO_FLOW_DEFAULT_BORDER"])) == (cfg["levels"], cfg["half_patch"], cfg["max_iter"], cfg["border"])
    assert (cfg["inverse"], cfg["early_stop"]) == (0, 0)
    assert float(val["VIO_FLOW_GRADIENT_DIVISOR"]) == fr.GRADIENT_DIVISOR == 26.0
    assert (int(val["VIO_FLOW_FAIL_LOST"]), int(val["VIO_FLOW_FAIL_BORDER"])) == (fr.FAIL_LOST, fr.FAIL_BORDER)
    back = {k: v for k, v in re.findall(r"(VIO_[A-Z_]+)\s*=\s*(-?[0-9]+)", open(os.path.join(ROOT, "include", "vio_backend.h")).read())}
    assert int(back["VIO_OK"]) == fr.OK and int(back["VIO_ERR_NOT_FINITE"]) == fr.NOT_FINITE


def test_python_binding_matches_the_header(vio):
    import ctypes as C
    from vio_amd import flow
    val = header_values()
    assert (flow.MAX_LEVELS, flow.MAX_HALF_PATCH, flow.MAX_POINTS, flow.MAX_DIM) == tuple(
        int(val["VIO_FLOW_" + k]) for k in ("MAX_LEVELS", "MAX_HALF_PATCH", "MAX_POINTS", "MAX_DIM"))
    assert (flow.DEFAULT_LEVELS, flow.DEFAULT_HALF_PATCH, flow.DEFAULT_MAX_ITER, flow.DEFAULT_BORDER) == tuple(
        int(val["VIO_FLOW_DEFAULT_" + k]) for k in ("LEVELS", "HALF_PATCH", "MAX_ITER", "BORDER"))
    assert (flow.FAIL_LOST, flow.FAIL_BORDER) == (int(val["VIO_FLOW_FAIL_LOST"]), int(val["VIO_FLOW_FAIL_BORDER"]))
    assert C.sizeof(flow.VioFlowPtInfo) == 16 and C.sizeof(flow.VioFlowConfig) == 24 and C.sizeof(flow.VioFlowItem) == 48


def test_handle_fails_with_a_status_without_a_gpu(vio):
    """On a machine without a GPU the create call returns a status (VioError), it does not crash; with one it succeeds."""
    lib = vio.load_flow()
    assert lib.fn["version"]() == 1
    try:
        h = lib.create()
    except vio.VioError as e:
        assert e.status in (-6, -2)
        return
    h.close()
