"""camera.parse_camodocal_yaml: the calibration text the reference's readFromYamlFile reads, into set_camera's keywords.  Four
settings-only fixtures under tests/golden/ (the PINHOLE one is the calibration block of the reference's config/euroc_config.yaml, the
others were written for this test with the key names the reference's CataCamera, EquidistantCamera and OCAMCamera read)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_reference as cr  # noqa: E402
from conftest import GOLDEN_DIR, load_package  # noqa: E402


def parse(name):
    return load_package().camera.parse_camodocal_yaml(open(os.path.join(GOLDEN_DIR, "camera_%s.yaml" % name)).read())


@pytest.mark.parametrize("name,expected", [("pinhole", cr.EUROC), ("mei", cr.MEI), ("scaramuzza", cr.SCARAMUZZA),
                                           ("kannala_brandt", {k: v for k, v in cr.KB_FOUR.items() if k != "theta_max"})])
def test_fixture_parses_into_the_keywords(name, expected):
    got = parse(name)
    assert got == expected, (got, expected)
    assert all(type(got[k]) is int for k in ("model", "width", "height"))
    # ... and the keywords are set_camera's: they fill the model's params[] without a complaint
    cam = load_package().camera
    p = cam.model_params(got["model"], **{k: v for k, v in got.items() if k not in ("model", "width", "height")})
    assert len(p) == len(cam.PARAMS[got["model"]]) <= cam.MAX_PARAMS
    cr.Camera(**got)


def test_unknown_model_type_is_refused():
    cam = load_package().camera
    text = open(os.path.join(GOLDEN_DIR, "camera_mei.yaml")).read()
    with pytest.raises(ValueError, match="model_type"):
        cam.parse_camodocal_yaml(text.replace("model_type: MEI", "model_type: DOUBLE_SPHERE"))
    with pytest.raises(ValueError, match="model_type"):
        cam.parse_camodocal_yaml(text.replace("model_type: MEI\n", ""))


def test_text_around_the_calibration_is_ignored():
    cam = load_package().camera
    text = open(os.path.join(GOLDEN_DIR, "camera_pinhole.yaml")).read()
    more = text + 'imu_topic: "/imu0"\nextrinsicRotation: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [0, -1, 0,\n          1, 0, 0,\n          0, 0, 1]\nestimate_extrinsic: 0   # 0  trusted\n'
    assert cam.parse_camodocal_yaml(more) == cam.parse_camodocal_yaml(text) == cr.EUROC


def test_missing_and_unknown_keywords_raise():
    cam = load_package().camera
    with pytest.raises(TypeError):
        cam.model_params(cam.MODEL_MEI, xi=1.0, gamma1=1.0, gamma2=1.0, u0=0.0)                 # v0 is missing
    with pytest.raises(TypeError):
        cam.model_params(cam.MODEL_PINHOLE, fx=1.0, fy=1.0, cx=0.0, cy=0.0, xi=1.0)              # PINHOLE has no xi
    with pytest.raises(ValueError):
        cam.model_params(7)
