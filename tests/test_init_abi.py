"""The surface of libvio_init_hip.so (include/vio_init.h): the header compiles as C99 and C++11 on its own, and the library exports
vio_init_* and nothing else of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vio_init.h")
LIB = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc", "libvio_init_hip.so")


@pytest.mark.parametrize("cc,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_alone(tmp_path, cc, std, ext):
    if not shutil.which(cc):
        pytest.fail("%s not found" % cc)
    src = tmp_path / ("t." + ext)
    src.write_text('#include "vio_init.h"\nint main(void) { vio_init_item it; vio_init_result r; (void)r; (void)it; return VIO_INIT_VERSION == 1 ? 0 : 1; }\n')
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.dirname(HDR), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_library_exports_only_vio_init():
    assert os.path.exists(LIB), "build first: %s" % LIB
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    own = [ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-2] in ("T", "D", "B", "R", "W", "V")]
    assert own and all(s.startswith("vio_init_") for s in own), own
    for s in ("vio_init_create", "vio_init_destroy", "vio_init_gyro_bias_batch", "vio_init_align_batch", "vio_init_timing",
              "vio_init_version", "vio_init_last_error"):
        assert s in own
