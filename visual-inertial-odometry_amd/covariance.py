"""ctypes binding of include/vio_covariance.h (csrc/libvio_cov_hip.so): marginal covariances of a solved window.

    cov = vio.load_cov()
    pose_cov, lm_var = ctx.covariance(w)                 # VioContext of the HIP library, w: the window passed to ctx.load()
    [(pose_cov, lm_var), ...] = hip.batch_covariance(ctxs, windows)     # many windows, one launch per kernel
    P_newest = vio.pose_block(pose_cov, vio.WINDOW_SIZE) # 6 x 6 covariance of the newest pose (position, rotation)

Ordering of pose_cov: [ext(6) | (pose 6, speed-bias 9) x 11] (vio_get_schur_system's); fixed variables are zero rows / columns.
"""
import ctypes as C

import numpy as np

from .capi import NUM_FRAMES, POSE_DIM, CompanionHandle, VioError, _dp, _f64, _ip, open_lib, window_field

GAUGE_NONE, GAUGE_FIX_OLDEST = 0, 1
GAUGES = {"none": GAUGE_NONE, "fix_oldest": GAUGE_FIX_OLDEST}


def pose_block(pose_cov, k):
    """The 6 x 6 covariance of frame k's pose (position, then rotation) out of a 171 x 171 pose_cov."""
    if not 0 <= k < NUM_FRAMES:
        raise IndexError("frame %d outside the window (0 .. %d)" % (k, NUM_FRAMES - 1))
    o = 6 + 15 * k
    return np.array(pose_cov[o:o + 6, o:o + 6])


def speed_bias_block(pose_cov, k):
    """The 9 x 9 covariance of frame k's speed and biases."""
    if not 0 <= k < NUM_FRAMES:
        raise IndexError("frame %d outside the window (0 .. %d)" % (k, NUM_FRAMES - 1))
    o = 12 + 15 * k
    return np.array(pose_cov[o:o + 9, o:o + 9])


class CovLib:
    """libvio_cov_hip.so: vio_cov_* (it resolves libvio_hip.so's symbols from the instance already loaded in the process)."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "compute", "compute_xyz", "compute_batch",
               "landmark_information", "pivot_ratio", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_cov_", self.SYMBOLS)
        self.fn["compute_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]

    def create(self, ctx):
        """A vio_cov handle bound to `ctx` (a VioContext of the HIP library)."""
        return CovHandle(self, ctx)

    def compute_batch(self, ctxs, windows, gauge="fix_oldest", out=None):
        """vio_cov_compute_batch over the windows of `ctxs` (VioContexts of the HIP library on one device and one stream, one kind of
        landmark), each with the handle VioContext.covariance uses.  windows: what each context was loaded with.  out: optional list
        of (pose_cov, lm) arrays to fill, one pair per window.  Returns one (pose_cov, lm) per window.
        A batch-level error raises VioError.  When some windows fail (VIO_ERR_NOT_FINITE) the others are still computed: the VioError
        raised then carries .window_status (every window's status), .results (None for a failed window) and names each failed window
        with its handle's message; a failed window's arrays are left untouched."""
        ctxs, windows = list(ctxs), list(windows)
        if len(ctxs) != len(windows):
            raise ValueError("%d contexts, %d windows" % (len(ctxs), len(windows)))
        B = len(ctxs)
        gi = GAUGES[gauge] if isinstance(gauge, str) else int(gauge)
        handles = [c.cov_handle() for c in ctxs]
        xyz0 = bool(B) and window_field(windows[0], "xyz") is not None          # the batch's kind: the library refuses a context holding the other
        items = (VioCovBatchItem * max(B, 1))()
        keep, res = [], []
        for i, (c, w) in enumerate(zip(ctxs, windows)):
            g = lambda k: window_field(w, k)
            n = c.n
            xyz = g("xyz") is not None
            P, L = out[i] if out is not None else (np.zeros((POSE_DIM, POSE_DIM)), np.zeros((n, 3, 3)) if xyz else np.zeros(n))
            assert P.shape == (POSE_DIM, POSE_DIM) and P.dtype == np.float64 and P.flags.c_contiguous
            assert L.dtype == np.float64 and L.flags.c_contiguous and L.size == n * (9 if xyz else 1)
            lm = np.ascontiguousarray(g("lm"), dtype=np.int32)
            m = lm.size
            if xyz:
                arrs = [lm, None, np.ascontiguousarray(g("frame"), dtype=np.int32), None, _f64(g("pts"), (m, 2))]
            else:
                arrs = [lm, np.ascontiguousarray(g("host"), dtype=np.int32), np.ascontiguousarray(g("target"), dtype=np.int32),
                        _f64(g("pts_i"), (m, 2)), _f64(g("pts_j"), (m, 2))]
            it = items[i]
            it.m, it.n = m, n
            it.lm, it.host, it.target, it.pts_i, it.pts_j = [a.ctypes.data if a is not None else None for a in arrs]
            it.pose_cov, it.lm_out = P.ctypes.data, (L.ctypes.data if n else None)
            keep.append(arrs)
            res.append((P, L))
        status = (C.c_int32 * max(B, 1))()
        hs = (C.c_void_p * max(B, 1))(*[h.h.value for h in handles])
        st = self.fn["compute_batch"](hs, C.c_int32(B), C.c_int32(gi), C.c_int32(1 if xyz0 else 0), items, status)
        if st == 0:
            return res
        if st != -3 or B == 0:
            handles[0]._ck(st, "compute_batch")
        ws = [int(status[i]) for i in range(B)]
        msgs = ["window %d: %s" % (i, (self.fn["last_error"](handles[i].h) or b"").decode(errors="replace"))
                for i in range(B) if ws[i] != 0]
        e = VioError(st, "vio_cov_compute_batch", "; ".join(msgs))
        e.window_status = ws
        e.results = [r if s == 0 else None for r, s in zip(res, ws)]
        raise e


class VioCovBatchItem(C.Structure):
    _fields_ = [("m", C.c_int64), ("lm", C.c_void_p), ("host", C.c_void_p), ("target", C.c_void_p), ("pts_i", C.c_void_p),
                ("pts_j", C.c_void_p), ("n", C.c_int64), ("pose_cov", C.c_void_p), ("lm_out", C.c_void_p)]


class CovHandle(CompanionHandle):
    PREFIX = "vio_cov_"

    def __init__(self, lib, ctx):
        self.lib = lib
        self.ctx = ctx
        self.h = C.c_void_p()
        st = lib.fn["create"](ctx.h, C.byref(ctx.cfg), C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_cov_create")


    def set_config(self, cfg):
        """vio_cov_set_config: the configuration the context now runs with (after VioContext.set_config)."""
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def pivot_ratio(self):
        """min_k d_k / S_kk of the last successful compute: near eps, the window barely constrains some direction."""
        r = C.c_double()
        self._ck(self.lib.fn["pivot_ratio"](self.h, C.byref(r)), "pivot_ratio")
        return r.value

    def compute(self, w, gauge="fix_oldest", pose_cov=None, lm_out=None):
        """(pose_cov (171, 171), lm_var (n,) or lm_cov (n, 3, 3)) of the context's current state.  w: the window passed to load().
        pose_cov / lm_out: optional arrays to fill (they are left untouched when the call fails)."""
        g = lambda k: window_field(w, k)
        gi = GAUGES[gauge] if isinstance(gauge, str) else int(gauge)
        xyz = g("xyz") is not None
        n = self.ctx.n
        P = np.zeros((POSE_DIM, POSE_DIM)) if pose_cov is None else pose_cov
        assert P.shape == (POSE_DIM, POSE_DIM) and P.dtype == np.float64 and P.flags.c_contiguous
        L = (np.zeros((n, 3, 3)) if xyz else np.zeros(n)) if lm_out is None else lm_out
        assert L.dtype == np.float64 and L.flags.c_contiguous and L.size == n * (9 if xyz else 1)
        Lp = _dp(L) if n else None
        lm = np.ascontiguousarray(g("lm"), dtype=np.int32)
        m = lm.size
        if xyz:
            fr = np.ascontiguousarray(g("frame"), dtype=np.int32)
            pts = _f64(g("pts"), (m, 2))
            st = self.lib.fn["compute_xyz"](self.h, C.c_int32(gi), C.c_int64(m), _ip(lm), _ip(fr), _dp(pts), C.c_int64(n), _dp(P), Lp)
            self._ck(st, "compute_xyz")
        else:
            host = np.ascontiguousarray(g("host"), dtype=np.int32)
            tgt = np.ascontiguousarray(g("target"), dtype=np.int32)
            pi, pj = _f64(g("pts_i"), (m, 2)), _f64(g("pts_j"), (m, 2))
            st = self.lib.fn["compute"](self.h, C.c_int32(gi), C.c_int64(m), _ip(lm), _ip(host), _ip(tgt), _dp(pi), _dp(pj),
                                        C.c_int64(n), _dp(P), Lp)
            self._ck(st, "compute")
        return P, L

    def landmark_information(self, xyz=False):
        """h_l (n,) or H_ll (n, 3, 3) as the last successful compute recomputed them."""
        n = self.ctx.n
        out = np.zeros((max(n, 1), 3, 3)) if xyz else np.zeros(max(n, 1))
        self._ck(self.lib.fn["landmark_information"](self.h, C.c_int64(n), _dp(out)), "landmark_information")
        return out[:n]

    def timing(self):
        """ms of the last compute: host (linearise + read-back + upload), k_cov_pose, k_cov_landmarks, whole call.  After a
        compute_batch: the batch's times, on every handle of the batch."""
        out = (C.c_double * 4)()
        self._ck(self.lib.fn["timing"](self.h, out), "timing")
        return {"host_ms": out[0], "k_cov_pose_ms": out[1], "k_cov_landmarks_ms": out[2], "total_ms": out[3]}
