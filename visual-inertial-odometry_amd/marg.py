"""ctypes binding of include/vio_marg.h (csrc/libvio_marg_hip.so): Problem::Marginalize for many windows in one call on the GPU.

    mh = vio.load_marg().create()                       # (device 0, its own stream; or stream=ctx.get_stream())
    prior = mh.compute(vio.MARG_OLD, w, w.prior)        # what ctx.load(w); ctx.marginalize(MARG_OLD) returns
    priors = mh.compute_batch([(kind, w, prior), ...])  # one upload, two launches, one read-back for the whole batch

w: a window as synth / StreamDriver.window_arrays make it (poses, speed_bias, ext, inv_depth, lm, host, target, pts_i, pts_j, preint);
prior: a dict with H (156 x 156) and b (156: vio_get_prior's b after a solve), or None.  Each result is the dict VioContext.marginalize
returns: H, b, err, jt_inv.
"""
import ctypes as C

import numpy as np

from .capi import MARG_OLD, MARG_SECOND_NEW, PRIOR_DIM, CompanionHandle, VioConfig, VioError, VioPreint, _f64, open_lib, window_field


class VioMargItem(C.Structure):
    _fields_ = [("kind", C.c_int32), ("poses", C.c_void_p), ("speed_bias", C.c_void_p), ("ext", C.c_void_p),
                ("n", C.c_int64), ("inv_depth", C.c_void_p), ("m", C.c_int64), ("lm", C.c_void_p), ("host", C.c_void_p),
                ("target", C.c_void_p), ("pts_i", C.c_void_p), ("pts_j", C.c_void_p), ("imu0", C.c_void_p),
                ("H_prior", C.c_void_p), ("b_prior", C.c_void_p),
                ("H", C.c_void_p), ("b", C.c_void_p), ("err", C.c_void_p), ("jt_inv", C.c_void_p)]


class MargLib:
    """libvio_marg_hip.so: vio_marg_*."""

    SYMBOLS = ["create", "set_config", "destroy", "last_error", "version", "compute_batch", "compute", "timing", "live_rows"]

    def __init__(self, path):
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_marg_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.POINTER(VioConfig), C.POINTER(C.c_void_p)]
        self.fn["set_config"].argtypes = [C.c_void_p, C.POINTER(VioConfig)]
        self.fn["compute_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["compute"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["live_rows"].argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]

    def create(self, cfg=None, **overrides):
        """A handle for `cfg` (a VioConfig, e.g. ctx.cfg of the contexts whose windows it marginalises; default: the library defaults
        of libvio_hip) with `overrides` applied (device, stream, loss_type, loss_delta, reproj_sqrt_info, gravity)."""
        if cfg is None:
            from . import load_hip
            cfg = load_hip().default_config()
        else:
            c2 = VioConfig()
            C.memmove(C.byref(c2), C.byref(cfg), C.sizeof(VioConfig))
            cfg = c2
        for k, v in overrides.items():
            if k == "gravity":
                for i in range(3):
                    cfg.gravity[i] = float(v[i])
            elif k == "stream":
                cfg.stream = v
            else:
                setattr(cfg, k, v)
        return MargHandle(self, cfg)


class MargHandle(CompanionHandle):
    PREFIX = "vio_marg_"

    def __init__(self, lib, cfg):
        self.lib, self.cfg = lib, cfg
        self.h = C.c_void_p()
        st = lib.fn["create"](C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_marg_create")

    def set_config(self, cfg):
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")
        self.cfg = cfg

    def _item(self, kind, w, prior, keep):
        it = VioMargItem()
        it.kind = int(kind)
        out = {"H": np.zeros((PRIOR_DIM, PRIOR_DIM)), "b": np.zeros(PRIOR_DIM), "err": np.zeros(PRIOR_DIM),
               "jt_inv": np.zeros((PRIOR_DIM, PRIOR_DIM))}
        keep.append(out)
        it.H, it.b, it.err, it.jt_inv = (out[k].ctypes.data for k in ("H", "b", "err", "jt_inv"))
        if prior is not None:
            H, b = _f64(prior["H"], (PRIOR_DIM, PRIOR_DIM)), _f64(np.asarray(prior["b"])[:PRIOR_DIM], (PRIOR_DIM,))
            keep += [H, b]
            it.H_prior, it.b_prior = H.ctypes.data, b.ctypes.data
        if w is not None and window_field(w, "xyz") is not None:
            raise VioError(-5, "vio_marg_compute", "XYZ landmarks: the reference's Estimator never marginalises them")
        if w is not None:
            arrs = {}
            for k, shape in (("poses", (11, 7)), ("speed_bias", (11, 9)), ("ext", (7,))):
                arrs[k] = _f64(window_field(w, k), shape)
            invd = _f64(window_field(w, "inv_depth"))
            lm = np.ascontiguousarray(window_field(w, "lm"), dtype=np.int32)
            host = np.ascontiguousarray(window_field(w, "host"), dtype=np.int32)
            target = np.ascontiguousarray(window_field(w, "target"), dtype=np.int32)
            m = len(lm)
            pi, pj = _f64(window_field(w, "pts_i"), (m, 2)), _f64(window_field(w, "pts_j"), (m, 2))
            keep += list(arrs.values()) + [invd, lm, host, target, pi, pj]
            it.poses, it.speed_bias, it.ext = arrs["poses"].ctypes.data, arrs["speed_bias"].ctypes.data, arrs["ext"].ctypes.data
            it.n, it.inv_depth = len(invd), (invd.ctypes.data if len(invd) else None)
            it.m = m
            if m:
                it.lm, it.host, it.target = lm.ctypes.data, host.ctypes.data, target.ctypes.data
                it.pts_i, it.pts_j = pi.ctypes.data, pj.ctypes.data
            pres = window_field(w, "preint")
            p0 = pres[0] if pres is not None and len(pres) else None
            if p0 is not None:
                p = VioPreint.from_dict(p0)
                keep.append(p)
                it.imu0 = C.addressof(p)
        return it, out

    def compute_batch(self, jobs, allow_nonfinite=False):
        """jobs: (kind, window, prior) triples.  Returns one prior dict per job.  A batch-level error raises VioError.  When some windows
        end VIO_ERR_NOT_FINITE, the others are still computed: without allow_nonfinite the VioError raised carries .window_status and
        .results (every window's dict, the failed ones holding the reference's outcome: H 0, the rest NaN)."""
        jobs = list(jobs)
        B = len(jobs)
        items = (VioMargItem * max(B, 1))()
        keep, res = [], []
        for i, (kind, w, prior) in enumerate(jobs):
            it, out = self._item(kind, w, prior, keep)
            items[i] = it
            res.append(out)
        ws = (C.c_int32 * max(B, 1))()
        st = self.lib.fn["compute_batch"](self.h, C.c_int32(B), C.cast(items, C.c_void_p), C.cast(ws, C.c_void_p))
        self.window_status = [int(ws[i]) for i in range(B)]
        if st == -3 and not allow_nonfinite:
            e = VioError(st, "vio_marg_compute_batch", self.last_error())
            e.window_status, e.results = self.window_status, res
            raise e
        if st not in (0, -3):
            self._ck(st, "compute_batch")
        return res

    def compute(self, kind, window, prior=None, allow_nonfinite=False):
        """One window (vio_marg_compute)."""
        keep = []
        it, out = self._item(kind, window, prior, keep)
        st = self.lib.fn["compute"](self.h, C.byref(it))
        if not (st == -3 and allow_nonfinite):
            self._ck(st, "compute")
        return out

    def timing(self):
        """[host pack + upload, k_marg_build, k_marg_tail, whole call] of the last call, ms."""
        t = np.zeros(4)
        self.lib.fn["timing"](self.h, t.ctypes.data)
        return t

    def live_rows(self, i=0):
        r = C.c_int32()
        st = self.lib.fn["live_rows"](self.h, C.c_int32(i), C.byref(r))
        if st != 0:
            raise VioError(st, "vio_marg_live_rows")
        return r.value
