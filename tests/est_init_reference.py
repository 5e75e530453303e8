"""A restatement of include/vio_est_init.h's two calls in Python floats over tests/est_reference.py: visualInitialAlign's writes into
the Estimator's own state (vins-mono/src/estimator.cpp:397-404, :419-425, :433, :444-455) from the rows the alignment wrote, and
IntegrationBase::repropagate (integration_base.h:38-52) for the intervals whose bias moved, which on a state that keeps an interval as
its samples and constructor arguments is a write of lin_bias[j].  Neither goes through atan2 / sin / cos, so both give the device's bits.

EstimatorInitReference is EstimatorReference with the two batched methods: the stand-in handle of the CPU driver tests.
"""
import math

import numpy as np

from est_reference import FRAMES, STATUS_OK, WINDOW_SIZE, EstimatorReference, F, apply33, copy_state, quat_to_rot

STATUS_NOT_READY = 2


def init_frame(pose, sb):
    """One frame: (Rs, Ps, Vs, Ba, Bg, lin_bias) from (p, q xyzw) and (V, ba, bg)."""
    x, y, z, w = pose[3:7]
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    Rs = quat_to_rot([x / n, y / n, z / n, w / n])
    return Rs, list(pose[0:3]), list(sb[0:3]), list(sb[3:6]), list(sb[6:9]), [0.0, 0.0, 0.0] + list(sb[6:9])


def init_apply(s, poses, sb, g, rot, commit_last=False):
    """vio_est_init_apply_batch for one slot; returns (new state, status).  A slot that is not ready is returned as it was."""
    if s["frame_count"] != WINDOW_SIZE or not all(int(e) != 0 for e in s["exists"][:FRAMES]):
        return s, STATUS_NOT_READY
    s = copy_state(s)
    poses, sb = np.asarray(poses, dtype=np.float64).reshape(FRAMES, 7), np.asarray(sb, dtype=np.float64).reshape(FRAMES, 9)
    for i in range(FRAMES):
        s["Rs"][i], s["Ps"][i], s["Vs"][i], s["Bas"][i], s["Bgs"][i], s["lin_bias"][i] = init_frame(F(poses[i]), F(sb[i]))
    s["g"] = np.array(apply33(F(rot), F(g)))
    if commit_last:
        s["last_R"], s["last_P"], s["last_R0"], s["last_P0"] = s["Rs"][10].copy(), s["Ps"][10].copy(), s["Rs"][0].copy(), s["Ps"][0].copy()
    return s, STATUS_OK


def relin_moved(Ba, Bg, lin, ba_thresh, bg_thresh):
    da = max(abs(Ba[c] - lin[c]) for c in range(3))
    dg = max(abs(Bg[c] - lin[3 + c]) for c in range(3))
    return da > ba_thresh or dg > bg_thresh


def relinearize(s, ba_thresh, bg_thresh):
    """vio_est_relinearize_batch for one slot; returns (new state, n_relinearized, mask)."""
    s = copy_state(s)
    mask = 0
    for j in range(1, FRAMES):
        if s["exists"][j] and relin_moved(F(s["Bas"][j - 1]), F(s["Bgs"][j - 1]), F(s["lin_bias"][j]), float(ba_thresh), float(bg_thresh)):
            s["lin_bias"][j] = np.concatenate([s["Bas"][j - 1], s["Bgs"][j - 1]])
            mask |= 1 << j
    return s, bin(mask).count("1"), mask


class EstimatorInitReference(EstimatorReference):
    """EstimatorReference with EstHandle.init_apply_batch and .relinearize_batch."""

    def init_apply_batch(self, items):
        out = []
        for slot, poses, sb, g, rot, *commit in items:
            vals = [np.asarray(v, dtype=np.float64) for v in (poses, sb, g, rot)]
            if not all(np.isfinite(v).all() for v in vals):
                raise ValueError("init_apply_batch: a non-finite entry")
            s, st = init_apply(self._s(slot), *vals, commit_last=bool(commit and commit[0]))
            self.state[slot] = s
            out.append(self._res(s, status=st))
        return out

    def relinearize_batch(self, items):
        out = []
        for slot, tba, tbg in items:
            if not (np.isfinite(tba) and np.isfinite(tbg) and tba >= 0 and tbg >= 0):
                raise ValueError("relinearize_batch: thresholds are finite and >= 0")
            s, n, mask = relinearize(self._s(slot), tba, tbg)
            self.state[slot] = s
            out.append(dict(status=STATUS_OK, frame_count=s["frame_count"], n_relinearized=n, mask=mask))
        return out
