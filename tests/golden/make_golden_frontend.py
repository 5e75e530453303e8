"""tests/golden/frontend_fixture.npz: what frontend.FeatureTracker (without a rejecter) gives on the fixture sequence of
tests/test_frontend_reference.py over the numpy tracker and detector: pts, ids (before and after update_ids) and track_cnt per frame.
It was recorded with the FeatureTracker that had no `rejecter` argument yet, and tests/test_frontend_reject.py holds today's
FeatureTracker(rejecter=None) to it byte for byte.

    python tests/golden/make_golden_frontend.py [path/to/frontend.py]      (default: the package's)
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import detect_reference as dr  # noqa: E402
from test_frontend_reference import MAX_CNT, MIN_DIST, Tracker, fixture_frames  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(HERE)), "visual-inertial-odometry_amd", "frontend.py")
    spec = importlib.util.spec_from_file_location("frontend_for_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ft = mod.FeatureTracker(Tracker(), dr.Detector(), max_cnt=MAX_CNT, min_dist=MIN_DIST)
    out = {}
    for t, img in enumerate(fixture_frames()):
        o = ft.read_image(img, 0.05 * t)
        for k in ("pts", "ids", "track_cnt"):
            out["%s_%d" % (k, t)] = o[k]
        out["ids_after_%d" % t] = ft.update_ids()
    np.savez_compressed(os.path.join(HERE, "frontend_fixture.npz"), **out)


if __name__ == "__main__":
    main()
