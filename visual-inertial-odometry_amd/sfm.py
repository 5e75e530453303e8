"""ctypes binding of include/vio_sfm.h (csrc/libvio_sfm_hip.so): structure-from-motion of many windows on the GPU.

    sh = vio.load_sfm().create()                             # (device 0, its own stream)
    rel = sh.relative_pose_batch(items)                      # relativePose + solveRelativeRT of every window: one dict per window
    out = sh.construct_batch(items, rel)                     # GlobalSFM::construct from those
    out = sh.sfm_batch(items)                                # both in one call; stage 1's dict under "rel"
    init_items = sfm_items_to_init_items(out, ric, pres)     # ImageFrame::R / T for InitHandle.initialize_batch

An item is a dict: n_frames F, start_frame (n_tracks,), obs_offset (n_tracks + 1,), pts (n_obs, 2): track j is seen in the consecutive
frames start_frame[j] .. with the normalised points pts[obs_offset[j] : obs_offset[j + 1]] (the CSR form vio_triangulate takes).
item_from_tracks makes one from a StreamDriver's tracks.
"""
import ctypes as C

import numpy as np

from .capi import CompanionHandle, VioError, open_lib

MAX_FRAMES = 16
MAX_TRACKS = 4096
DEFAULT_HYPOTHESES = 128
OK, NOT_FINITE = 0, -3
FAIL_RELATIVE_POSE, FAIL_PNP, FAIL_BA = 1, 2, 3
# StreamDriver(initialize=dict(sfm=...)): the `status` of a try whose SfM failed is TRY_FAILED_SFM + |SfM status| (101, 102, 103; 103
# also for a non-finite window), above every VIO_INIT_FAIL_* code of the alignment; the SfM status itself is under `sfm_status`
TRY_FAILED_SFM = 100
STATUS_NAMES = {OK: "ok", NOT_FINITE: "not finite", FAIL_RELATIVE_POSE: "relativePose: no frame with enough correspondences, parallax "
                "and points in front", FAIL_PNP: "solveFrameByPnP failed", FAIL_BA: "the bundle adjustment did not converge"}


class VioSfmConfig(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("ransac_hypotheses", C.c_int32)]


class VioSfmItem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_tracks", C.c_int32), ("start_frame", C.c_void_p), ("obs_offset", C.c_void_p),
                ("pts", C.c_void_p)]


class VioSfmRelResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("l", C.c_int32), ("hyp", C.c_int32), ("n_corres", C.c_int32), ("n_inliers", C.c_int32),
                ("n_front", C.c_int32), ("R", C.c_double * 9), ("T", C.c_double * 3), ("corres", C.c_int32 * MAX_FRAMES),
                ("parallax", C.c_double * MAX_FRAMES)]


class VioSfmResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("fail_frame", C.c_int32), ("ba_iterations", C.c_int32), ("ba_converged", C.c_int32),
                ("n_triangulated", C.c_int32), ("pnp_iterations", C.c_int32 * MAX_FRAMES), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("Q", C.c_double * (4 * MAX_FRAMES)), ("T", C.c_double * (3 * MAX_FRAMES))]


class SfmLib:
    """libvio_sfm_hip.so: vio_sfm_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "relative_pose_batch", "construct_batch", "batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_sfm_", self.SYMBOLS)
        self.fn["sfm_batch"] = self.fn["batch"]
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["relative_pose_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["construct_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_sfm handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return SfmHandle(self, device, stream)


class _Packed:
    """The ctypes items of a batch and the arrays they point into (kept alive as long as the items)."""

    def __init__(self, items):
        self.keep = []
        self.items = (VioSfmItem * max(1, len(items)))()
        self.nt = []
        for i, it in enumerate(items):
            sf = np.ascontiguousarray(it["start_frame"], dtype=np.int32)
            off = np.ascontiguousarray(it["obs_offset"], dtype=np.int64)
            pts = np.ascontiguousarray(it["pts"], dtype=np.float64).reshape(-1, 2)
            if off.size != sf.size + 1 or (off.size and off[-1] != len(pts)):
                raise ValueError("window %d: obs_offset must have n_tracks + 1 entries and end at len(pts)" % i)
            self.keep += [sf, off, pts]
            self.nt.append(int(sf.size))
            self.items[i] = VioSfmItem(int(it["n_frames"]), int(sf.size), sf.ctypes.data, off.ctypes.data, pts.ctypes.data)
        self.total = sum(self.nt)
        self.base = np.concatenate([[0], np.cumsum(self.nt)]).astype(np.int64)


def _rel_dict(r, F, mask):
    return dict(status=int(r.status), l=int(r.l), hyp=int(r.hyp), n_corres=int(r.n_corres), n_inliers=int(r.n_inliers),
                front=int(r.n_front), R=np.array(r.R[:]).reshape(3, 3), T=np.array(r.T[:]), corres=np.array(r.corres[:F - 1]),
                parallax=np.array(r.parallax[:F - 1]), mask=mask)


def _res_dict(r, F, points, state):
    return dict(status=int(r.status), fail_frame=int(r.fail_frame), ba_iterations=int(r.ba_iterations),
                ba_converged=bool(r.ba_converged), n_triangulated=int(r.n_triangulated),
                pnp_iterations=np.array(r.pnp_iterations[:F]), initial_cost=r.initial_cost, final_cost=r.final_cost,
                Q=np.array(r.Q[:4 * F]).reshape(F, 4), T=np.array(r.T[:3 * F]).reshape(F, 3), points=points, state=state)


class SfmHandle(CompanionHandle):
    PREFIX = "vio_sfm_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_sfm_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def set_config(self, seed=0, ransac_hypotheses=DEFAULT_HYPOTHESES):
        cfg = VioSfmConfig(int(seed), int(ransac_hypotheses))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def relative_pose_batch(self, items):
        """relativePose + solveRelativeRT of every window: a list of dicts (status, l, hyp, n_corres, n_inliers, front, R (3 x 3) =
        relative_R, T = relative_T, corres / parallax (F - 1 candidates), mask (n_corres,) bool).  Non-finite windows do not raise."""
        B = len(items)
        pk = _Packed(items)
        rel = (VioSfmRelResult * max(B, 1))()
        mask = np.zeros(max(pk.total, 1), dtype=np.uint8)
        st = self.lib.fn["relative_pose_batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(rel), mask.ctypes.data)
        self._ck(st, "relative_pose_batch", allow_not_finite=True)
        return [_rel_dict(rel[i], int(items[i]["n_frames"]), mask[pk.base[i]:pk.base[i] + max(rel[i].n_corres, 0)].astype(bool))
                for i in range(B)]

    @staticmethod
    def _pack_rel(rels):
        rel = (VioSfmRelResult * max(len(rels), 1))()
        for i, r in enumerate(rels):
            rel[i].status, rel[i].l = int(r["status"]), int(r["l"])
            rel[i].R[:] = list(np.asarray(r["R"], dtype=np.float64).reshape(9))
            rel[i].T[:] = list(np.asarray(r["T"], dtype=np.float64).reshape(3))
        return rel

    def construct_batch(self, items, rels):
        """GlobalSFM::construct of every window from stage 1's dicts (status, l, R, T are read): a list of dicts (status, fail_frame,
        Q (F, 4) wxyz, T (F, 3), points (n_tracks, 3), state (n_tracks,) bool, pnp_iterations (F,), ba_iterations, ba_converged,
        n_triangulated, initial_cost, final_cost)."""
        B = len(items)
        pk = _Packed(items)
        rel = self._pack_rel(rels)
        res = (VioSfmResult * max(B, 1))()
        points = np.full((max(pk.total, 1), 3), np.nan)
        state = np.zeros(max(pk.total, 1), dtype=np.uint8)
        st = self.lib.fn["construct_batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(rel), C.addressof(res),
                                            points.ctypes.data, state.ctypes.data)
        self._ck(st, "construct_batch", allow_not_finite=True)
        return [_res_dict(res[i], int(items[i]["n_frames"]), points[pk.base[i]:pk.base[i + 1]].copy(),
                          state[pk.base[i]:pk.base[i + 1]].astype(bool)) for i in range(B)]

    def sfm_batch(self, items):
        """Both stages in one call: construct_batch's dicts, each with stage 1's dict under "rel"."""
        B = len(items)
        pk = _Packed(items)
        rel = (VioSfmRelResult * max(B, 1))()
        res = (VioSfmResult * max(B, 1))()
        mask = np.zeros(max(pk.total, 1), dtype=np.uint8)
        points = np.full((max(pk.total, 1), 3), np.nan)
        state = np.zeros(max(pk.total, 1), dtype=np.uint8)
        st = self.lib.fn["batch"](self.h, C.c_int32(B), C.addressof(pk.items), C.addressof(rel), mask.ctypes.data, C.addressof(res),
                                  points.ctypes.data, state.ctypes.data)
        self._ck(st, "sfm_batch", allow_not_finite=True)
        out = []
        for i in range(B):
            F = int(items[i]["n_frames"])
            d = _res_dict(res[i], F, points[pk.base[i]:pk.base[i + 1]].copy(), state[pk.base[i]:pk.base[i + 1]].astype(bool))
            d["rel"] = _rel_dict(rel[i], F, mask[pk.base[i]:pk.base[i] + max(rel[i].n_corres, 0)].astype(bool))
            out.append(d)
        return out

    def timing(self):
        """ms of the last call: host packing + upload, k_sfm_relpose, k_sfm_construct (NaN for a stage that did not run), the whole call."""
        t = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"host_ms": t[0], "relpose_ms": t[1], "construct_ms": t[2], "total_ms": t[3]}


def item_from_tracks(tracks, frames):
    """The SfM item of a StreamDriver's tracks (landmark -> [(global frame, point)] over consecutive window frames) for the window
    `frames`, in the dict's order (sfm_f, estimator.cpp:275-289).  Returns (item, landmark ids)."""
    sf, off, pts, ids = [], [0], [], []
    for lm, tr in tracks.items():
        sf.append(frames.index(tr[0][0]))
        pts.extend(p for _, p in tr)
        off.append(off[-1] + len(tr))
        ids.append(lm)
    return dict(n_frames=len(frames), start_frame=np.array(sf, dtype=np.int32), obs_offset=np.array(off, dtype=np.int64),
                pts=np.array(pts, dtype=np.float64).reshape(-1, 2)), ids


def quat_wxyz_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def sfm_items_to_init_items(results, ric, pres, is_key=None):
    """The alignment items of successful SfM results, as initialStructure leaves the keyframes (estimator.cpp:316-318):
    ImageFrame::R = Q * RIC^T, ImageFrame::T = T.  results: sfm_batch's (or construct_batch's) dicts; ric: RIC[0] (3 x 3); pres[i]:
    window i's F - 1 pre-integration records.  A window that did not succeed gives None."""
    ric = np.asarray(ric, dtype=np.float64).reshape(3, 3)
    out = []
    for i, r in enumerate(results):
        if r["status"] != OK:
            out.append(None)
            continue
        R = np.stack([quat_wxyz_to_rot(q) @ ric.T for q in r["Q"]])
        out.append(dict(R=R, T=np.asarray(r["T"], dtype=np.float64).copy(), pre=list(pres[i]), is_key=is_key))
    return out
