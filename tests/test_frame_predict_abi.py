"""The surface of the prediction in the resident-frame library (include/vio_frame_predict.h, libvio_frame_hip.so), in the manner of
tests/test_frame_back_abi.py: the header compiles alone as C99 and C++11, include/vio_frame.h brings it in behind vio_frame_back.h and
declares nothing new itself, the library exports exactly the four new names beside the old ones and the binding agrees with the header."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
HEADER, LIB, PREFIX = "vio_frame_predict.h", "libvio_frame_hip.so", "vio_frame_"
NAMES = {"vio_frame_set_prediction_batch", "vio_frame_clear_prediction", "vio_frame_set_prediction_fallback", "vio_frame_read_predict_info"}
OLDER = ("vio_frame.h", "vio_frame_read.h", "vio_frame_camera.h", "vio_frame_back.h")
BODY = ("vio_frame_prediction_item p; vio_frame_read_result r; (void)p; (void)r; "
        "return VIO_FRAME_VERSION == 1 && VIO_FRAME_HAS_PREDICT == 1 && VIO_FRAME_HAS_BACK == 1 && VIO_FRAME_MAX_TRACK_POINTS == 1024 && "
        "sizeof(vio_frame_read_result) == 40 && sizeof(vio_frame_prediction_item) == 8 + 2 * sizeof(void *) ? 0 : 1;")


def declared(header=HEADER):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % PREFIX, txt)))


@pytest.mark.parametrize("header", [HEADER, "vio_frame.h"])
@pytest.mark.parametrize("cc,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_alone(tmp_path, cc, std, ext, header):
    if not shutil.which(cc):
        pytest.fail("%s not found" % cc)
    src = tmp_path / ("t." + ext)
    src.write_text('#include "%s"\nint main(void) { %s }\n' % (header, BODY))
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])
    exe = tmp_path / "t"
    subprocess.check_call([cc, str(tmp_path / "t.o"), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_library_exports_exactly_the_new_names_beside_the_old():
    lib = os.path.join(CSRC, LIB)
    assert os.path.exists(lib), "build first: %s" % lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    own = [ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-2] in ("T", "D", "B", "R", "W", "V")]
    assert own and all(s.startswith(PREFIX) for s in own), own
    assert set(declared()) == NAMES
    older = set(s for hdr in OLDER for s in declared(hdr))
    assert not older & NAMES and set(own) == older | NAMES, sorted(set(own) ^ (older | NAMES))
    # include/vio_frame.h declares what it declared, and brings the new header in behind vio_frame_back.h
    txt = open(os.path.join(ROOT, "include", "vio_frame.h")).read()
    assert "#define VIO_FRAME_HAS_PREDICT 1" in txt and "#define VIO_FRAME_VERSION 1\n" in txt
    assert txt.index('#include "vio_frame_back.h"') < txt.index('#include "vio_frame_predict.h"')
    script = open(os.path.join(CSRC, "libvio_frame_hip.map")).read()
    assert "global: vio_frame_*;" in script and "local: *;" in script


def test_the_non_finite_deviation_is_recorded_in_the_header():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "not finite is refused" in txt and "VIO_ERR_NOT_FINITE" in txt


def test_python_binding_matches_the_header(vio):
    import ctypes as C
    from vio_amd import frame, frontend
    assert sorted(PREFIX + s for s in frame.FrameLib.PREDICT_SYMBOLS) == sorted(NAMES)
    assert C.sizeof(frame.VioFramePredictionItem) == 24
    lib = vio.load_frame()
    assert all(lib.fn[s] is not None for s in frame.FrameLib.PREDICT_SYMBOLS)
    for m in ("set_prediction_batch", "clear_prediction", "set_prediction_fallback", "read_predict_info"):
        assert callable(getattr(frame.FrameHandle, m)), m
    p = inspect.signature(frontend.BatchFeatureTracker.__init__).parameters
    assert p["prediction"].default is None
    assert callable(frontend.BatchFeatureTracker.set_predictions) and callable(frontend.predict_pixels_batch)


def test_calls_without_a_handle_return_a_status(vio):
    """The four calls check their handle before anything else: no device is needed to be refused."""
    fn = vio.load_frame().fn
    assert fn["set_prediction_batch"](None, 0, None) == -1 and fn["clear_prediction"](None, 0) == -1
    assert fn["set_prediction_fallback"](None, 0) == -1 and fn["read_predict_info"](None, 0, None, None, None, None) == -1
