"""Writes tests/golden/sfm_sampling.npz: the 8 sample indices of a few (seed, i, h, n) under the hash of include/vio_sfm.h, from
tests/sfm_reference.sample8.  The file pins the hash: a change to it changes every RANSAC result."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sfm_reference as sr  # noqa: E402

keys = [(0, 0, 0, 8), (0, 0, 0, 30), (0, 0, 1, 30), (0, 5, 127, 40), (1, 0, 0, 30), (12345, 9, 4095, 1000), (0xFFFFFFFF, 14, 7, 9),
        (7, 3, 64, 21)]
np.savez(os.path.join(HERE, "sfm_sampling.npz"), keys=np.array(keys, dtype=np.int64),
         indices=np.array([sr.sample8(*k) for k in keys], dtype=np.int32),
         hashes=np.array([sr.hash4(k[0], k[1], k[2], 0) for k in keys], dtype=np.int64))
