"""ctypes binding of include/vio_residuals.h (csrc/libvio_res_hip.so): per-edge residuals, the chi2 breakdown and landmark outlier
flags of a window.

    r = ctx.residuals(w)                 # VioContext of the HIP library, w: the window passed to ctx.load()
    r["obs"]      (m, 4)  r_x, r_y, e2, rho0 per edge, in w's order
    r["lm"]       (n, 3)  mean and max pixel error, sum of rho0 per landmark
    r["flags"]    (n,)    uint8: FLAG_REPROJ | FLAG_DEPTH | FLAG_STATE
    r["summary"]  dict    chi2, visual_robust, visual_plain, imu, prior, imu_edge (10), frame_robust (11), frame_edges (11), n_flagged (3)
    [r, ...] = hip.batch_residuals(ctxs, windows)        # many windows, one launch per kernel
"""
import ctypes as C

import numpy as np

from . import synth
from .capi import NUM_FRAMES, WINDOW_SIZE, CompanionHandle, VioError, _f64, open_lib, preint_pointers, window_field

FLAG_REPROJ, FLAG_DEPTH, FLAG_STATE = 1, 2, 4
FLAGS_ALL = FLAG_REPROJ | FLAG_DEPTH | FLAG_STATE


class VioResSummary(C.Structure):
    _fields_ = [("chi2", C.c_double), ("visual_robust", C.c_double), ("visual_plain", C.c_double), ("imu", C.c_double),
                ("prior", C.c_double), ("imu_edge", C.c_double * WINDOW_SIZE), ("frame_robust", C.c_double * NUM_FRAMES),
                ("frame_edges", C.c_int64 * NUM_FRAMES), ("n_flagged", C.c_int64 * 3)]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = np.array(v[:]) if hasattr(v, "_length_") else float(v)
        return out


class ResLib:
    """libvio_res_hip.so: vio_res_* (it resolves libvio_hip.so's symbols from the instance already loaded in the process)."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set_config", "compute", "compute_xyz", "compute_batch", "timing"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_res_", self.SYMBOLS)
        self.fn["compute"].argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 4
        self.fn["compute_xyz"].argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 4
        self.fn["compute_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_double]

    def create(self, ctx):
        """A vio_res handle bound to `ctx` (a VioContext of the HIP library)."""
        return ResHandle(self, ctx)

    def compute_batch(self, ctxs, windows, focal=synth.FOCAL, outlier_px=3.0, outputs=("obs", "lm", "flags", "summary"), out=None,
                      imu=True):
        """vio_res_compute_batch over the windows of `ctxs` (VioContexts of the HIP library on one device and one stream, one kind of
        landmark), each with the handle VioContext.residuals uses.  windows: what each context was loaded with.  outputs / imu: as
        ResHandle.compute, for every window; out: optional list of such dicts of caller-owned arrays, one per window.  Returns one
        dict per window, in ResHandle.compute's shape.  Errors raise VioError (nothing is written then)."""
        ctxs, windows = list(ctxs), list(windows)
        if len(ctxs) != len(windows):
            raise ValueError("%d contexts, %d windows" % (len(ctxs), len(windows)))
        B = len(ctxs)
        handles = [c.res_handle() for c in ctxs]
        xyz0 = bool(B) and window_field(windows[0], "xyz") is not None          # the batch's kind: the library refuses a context holding the other
        items = (VioResBatchItem * max(B, 1))()
        keep, res = [], []
        want = set(outputs)
        for i, (c, w) in enumerate(zip(ctxs, windows)):
            g = lambda k: window_field(w, k)
            n = c.n
            lm = np.ascontiguousarray(g("lm"), dtype=np.int32)
            m = lm.size
            if m != c.m:
                raise VioError(-1, "vio_res_compute_batch", "(window %d has %d edges, its context %d)" % (i, m, c.m))
            if g("xyz") is not None:
                arrs = [lm, None, np.ascontiguousarray(g("frame"), dtype=np.int32), None, _f64(g("pts"), (m, 2))]
            else:
                arrs = [lm, np.ascontiguousarray(g("host"), dtype=np.int32), np.ascontiguousarray(g("target"), dtype=np.int32),
                        _f64(g("pts_i"), (m, 2)), _f64(g("pts_j"), (m, 2))]
            o = dict((out[i] if out is not None else None) or {})
            outs = {}
            if "obs" in want:
                outs["obs"] = o.get("obs", np.zeros((m, 4)))
            if "lm" in want:
                outs["lm"] = o.get("lm", np.zeros((n, 3)))
            if "flags" in want:
                outs["flags"] = o.get("flags", np.zeros(n, dtype=np.uint8))
            for a in outs.values():
                assert a.flags.c_contiguous
            summ = VioResSummary() if "summary" in want else None
            pre = _pre_array(g("preint")) if imu else (None, None)
            it = items[i]
            it.m, it.n = m, n
            it.lm, it.host, it.target, it.pts_i, it.pts_j = [a.ctypes.data if a is not None else None for a in arrs]
            it.pre = C.addressof(pre[0]) if pre[0] is not None else None
            ptr = lambda k: outs[k].ctypes.data if k in outs and outs[k].size else None
            it.obs_out, it.lm_out, it.lm_flags = ptr("obs"), ptr("lm"), ptr("flags")
            it.summary = C.addressof(summ) if summ is not None else None
            keep.append((arrs, pre))
            res.append((outs, summ))
        hs = (C.c_void_p * max(B, 1))(*[h.h.value for h in handles])
        st = self.fn["compute_batch"](hs, C.c_int32(B), C.c_int32(1 if xyz0 else 0), items, C.c_double(focal), C.c_double(outlier_px))
        if B:
            handles[0]._ck(st, "compute_batch")
        elif st != 0:
            raise VioError(st, "vio_res_compute_batch")
        out_list = []
        for outs, summ in res:
            r = {k: outs.get(k) for k in ("obs", "lm", "flags")}
            r["summary"] = summ.as_dict() if summ is not None else None
            out_list.append(r)
        return out_list


class VioResBatchItem(C.Structure):
    _fields_ = [("m", C.c_int64), ("lm", C.c_void_p), ("host", C.c_void_p), ("target", C.c_void_p), ("pts_i", C.c_void_p),
                ("pts_j", C.c_void_p), ("n", C.c_int64), ("pre", C.c_void_p), ("obs_out", C.c_void_p), ("lm_out", C.c_void_p),
                ("lm_flags", C.c_void_p), ("summary", C.c_void_p)]


def _pre_array(pres):
    """The ten pointers of vio_set_imu_all (None: no edge) and the structs they point to (kept alive by the caller)."""
    pres = list(pres)
    if len(pres) != WINDOW_SIZE:
        raise ValueError("the window's %d IMU edges (None for a missing one), got %d" % (WINDOW_SIZE, len(pres)))
    return preint_pointers(pres)


class ResHandle(CompanionHandle):
    PREFIX = "vio_res_"

    def __init__(self, lib, ctx):
        self.lib = lib
        self.ctx = ctx
        self.h = C.c_void_p()
        st = lib.fn["create"](ctx.h, C.byref(ctx.cfg), C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_res_create")


    def set_config(self, cfg):
        """vio_res_set_config: the configuration the context now runs with (after VioContext.set_config)."""
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def compute(self, w, focal=synth.FOCAL, outlier_px=3.0, n=None, outputs=("obs", "lm", "flags", "summary"), out=None, imu=True):
        """The residual query at the context's current state.  w: the window passed to load().  n: the landmark count passed to the
        library (default: the context's).  outputs: which outputs to ask for (the others are passed as NULL and come back None).
        out: optional dict of caller-owned arrays to fill ("obs" (m, 4), "lm" (n, 3), "flags" (n,) uint8); they are left untouched
        when the call fails.  imu=False passes pre = NULL (the IMU terms and chi2 come back NaN)."""
        g = lambda k: window_field(w, k)
        xyz = g("xyz") is not None
        n = self.ctx.n if n is None else int(n)
        lm = np.ascontiguousarray(g("lm"), dtype=np.int32)
        m = lm.size
        if m != self.ctx.m:
            raise VioError(-1, "vio_res_compute", "(the window has %d edges, the context %d)" % (m, self.ctx.m))
        out = dict(out or {})
        want = set(outputs)
        arrs = {}
        if "obs" in want:
            arrs["obs"] = out.get("obs", np.zeros((m, 4)))
        if "lm" in want:
            arrs["lm"] = out.get("lm", np.zeros((max(n, 0), 3)))
        if "flags" in want:
            arrs["flags"] = out.get("flags", np.zeros(max(n, 0), dtype=np.uint8))
        for a in arrs.values():
            assert a.flags.c_contiguous
        summ = VioResSummary() if "summary" in want else None
        ptr = lambda k: arrs[k].ctypes.data if k in arrs and arrs[k].size else None
        pre, _keep = _pre_array(g("preint")) if imu else (None, None)
        tail = [C.c_int64(n), pre, C.c_double(focal), C.c_double(outlier_px), ptr("obs"), ptr("lm"), ptr("flags"),
                C.addressof(summ) if summ is not None else None]
        if xyz:
            fr = np.ascontiguousarray(g("frame"), dtype=np.int32)
            pts = _f64(g("pts"), (m, 2))
            st = self.lib.fn["compute_xyz"](self.h, C.c_int64(m), lm.ctypes.data, fr.ctypes.data, pts.ctypes.data, *tail)
            self._ck(st, "compute_xyz")
        else:
            host = np.ascontiguousarray(g("host"), dtype=np.int32)
            tgt = np.ascontiguousarray(g("target"), dtype=np.int32)
            pi, pj = _f64(g("pts_i"), (m, 2)), _f64(g("pts_j"), (m, 2))
            st = self.lib.fn["compute"](self.h, C.c_int64(m), lm.ctypes.data, host.ctypes.data, tgt.ctypes.data, pi.ctypes.data,
                                        pj.ctypes.data, *tail)
            self._ck(st, "compute")
        res = {k: arrs.get(k) for k in ("obs", "lm", "flags")}
        res["summary"] = summ.as_dict() if summ is not None else None
        return res

    def timing(self):
        """ms of the last compute: host (read-back of the states + packing + upload), the three kernels, whole call.  After a
        compute_batch: the batch's times, on every handle of the batch."""
        out = (C.c_double * 5)()
        self._ck(self.lib.fn["timing"](self.h, out), "timing")
        return {"host_ms": out[0], "k_res_obs_ms": out[1], "k_res_lm_ms": out[2], "k_res_tail_ms": out[3], "total_ms": out[4]}
