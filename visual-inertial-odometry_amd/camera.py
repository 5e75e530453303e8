"""ctypes binding of include/vio_camera.h (csrc/libvio_camera_hip.so): the lift, undistortedPoints and rejectWithF through the
reference's four camera models (PINHOLE, KANNALA_BRANDT, MEI, SCARAMUZZA), for many streams with a camera each on the GPU.

    ch = vio.load_camera().create()                                  # (device 0, its own stream)
    ch.set_camera(slot=0, model=camera.MODEL_KANNALA_BRANDT, width=752, height=480, k2=.., k3=.., k4=.., k5=.., mu=.., mv=.., u0=.., v0=..)
    ch.set_camera(**camera.parse_camodocal_yaml(open("fisheye.yaml").read()))          # ... or from the reference's calibration text
    ch.set_config(seed=0, ransac_hypotheses=128, f_threshold=1.0, focal_length=460.0)
    keep = ch.reject(cur_pts, forw_pts, pair)                        # RejectHandle's interface, on the default slot
    un, vel = ch.undistort(pts, ids, prev_ids, prev_un_pts, dt)
    rays = ch.lift(pts)                                              # (n, 3) float64
    outs = ch.lift_batch([dict(pts=, slot=), ...])                   # dicts: status, n_clamped, rays (n, 3), angles (n, 2)
    outs = ch.undistort_batch([dict(pts=, ids=, prev_ids=, prev_un_pts=, dt=, slot=), ...])   # status, n_clamped, un_pts, velocity
    outs = ch.reject_batch([dict(cur_pts=, forw_pts=, pair=, slot=), ...])                    # status, hyp, n_inliers, F, mask
    other = ch.bind(3)                                               # the same handle with slot 3 as its default slot
    ch.set_inv_poly(slot, coeffs)                                    # SCARAMUZZA's inv_poly_parameters (include/vio_camera_project.h)
    pixels = ch.project(points, slot=0)                              # spaceToPlane: (n, 3) float64 -> (n, 2) float64
    outs = ch.project_batch([dict(points=, slot=), ...])             # dicts: status, n_flagged, pixels (n, 2), flags (n,) uint8

A CameraHandle (or a bind() view) is a FeatureTracker rejecter: FeatureTracker(rejecter=ch, frames=, slot=).  An item whose lift the
tracker cannot use (a pixel that is not finite, P2 == 0 on a fisheye) gets status NOT_FINITE and does not raise.
"""
import ctypes as C
import math

import numpy as np

from .capi import CompanionHandle, VioError
from .reject import (DEFAULT_F_THRESHOLD, DEFAULT_FOCAL_LENGTH, DEFAULT_HYPOTHESES, FAIL_NO_MODEL, NOT_FINITE, OK, VioRejectConfig,
                     VioRejectResult, _ids, _pts)

MAX_SLOTS, MAX_PARAMS, MAX_POINTS, MAX_ITEMS = 256, 16, 4096, 4096
KB_BISECTIONS, KB_NEWTON, KB_GRID = 12, 8, 4096
KB_DEFAULT_THETA_MAX = math.pi
KB_RAY_C = 3.6
INV_POLY_MAX = 20                                                      # include/vio_camera_project.h
PROJECT_NOT_FINITE, PROJECT_BEHIND = 1, 2
PROJECT_C = 3e-13
MODEL_PINHOLE, MODEL_KANNALA_BRANDT, MODEL_MEI, MODEL_SCARAMUZZA = 0, 1, 2, 3
MODEL_NAMES = {"PINHOLE": MODEL_PINHOLE, "KANNALA_BRANDT": MODEL_KANNALA_BRANDT, "MEI": MODEL_MEI, "SCARAMUZZA": MODEL_SCARAMUZZA}

# params[] of vio_camera_model per model, in the order the reference's readFromYamlFile reads them; (name, default)
PARAMS = {
    MODEL_PINHOLE: [("k1", 0.0), ("k2", 0.0), ("p1", 0.0), ("p2", 0.0), ("fx", None), ("fy", None), ("cx", None), ("cy", None)],
    MODEL_MEI: [("xi", None), ("k1", 0.0), ("k2", 0.0), ("p1", 0.0), ("p2", 0.0), ("gamma1", None), ("gamma2", None), ("u0", None), ("v0", None)],
    MODEL_SCARAMUZZA: [("poly0", None), ("poly1", 0.0), ("poly2", 0.0), ("poly3", 0.0), ("poly4", 0.0), ("ac", 1.0), ("ad", 0.0), ("ae", 0.0),
                       ("cx", None), ("cy", None)],
    MODEL_KANNALA_BRANDT: [("k2", 0.0), ("k3", 0.0), ("k4", 0.0), ("k5", 0.0), ("mu", None), ("mv", None), ("u0", None), ("v0", None),
                           ("theta_max", KB_DEFAULT_THETA_MAX)],
}


class VioCameraModel(C.Structure):
    _fields_ = [("model", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32), ("params", C.c_double * MAX_PARAMS)]


class VioCameraLiftItem(C.Structure):
    _fields_ = [("n", C.c_int32), ("slot", C.c_int32), ("pts", C.c_void_p), ("rays", C.c_void_p), ("angles", C.c_void_p)]


class VioCameraLiftResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_clamped", C.c_int32)]


class VioCameraUndistortItem(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("pts", C.c_void_p), ("ids", C.c_void_p), ("prev_ids", C.c_void_p),
                ("prev_un_pts", C.c_void_p), ("dt", C.c_double), ("un_pts", C.c_void_p), ("velocity", C.c_void_p),
                ("slot", C.c_int32), ("reserved", C.c_int32)]


class VioCameraRejectItem(C.Structure):
    _fields_ = [("n", C.c_int32), ("pair", C.c_uint32), ("cur_pts", C.c_void_p), ("forw_pts", C.c_void_p), ("slot", C.c_int32),
                ("reserved", C.c_int32)]


class VioCameraProjectItem(C.Structure):                                # include/vio_camera_project.h
    _fields_ = [("n", C.c_int32), ("slot", C.c_int32), ("points", C.c_void_p), ("pixels", C.c_void_p), ("flags", C.c_void_p)]


class VioCameraProjectResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_flagged", C.c_int32)]


def model_params(model, **params):
    """The params[] array of `model` from keywords named as the reference's calibration files name them (SCARAMUZZA's polynomial is
    poly0 .. poly4).  A missing keyword without a default and an unknown keyword raise."""
    if model not in PARAMS:
        raise ValueError("unknown camera model %r" % (model,))
    out, left = [], dict(params)
    for name, default in PARAMS[model]:
        v = left.pop(name, default)
        if v is None:
            raise TypeError("camera model %d needs %s" % (model, name))
        out.append(float(v))
    if left:
        raise TypeError("camera model %d takes no %s" % (model, ", ".join(sorted(left))))
    return out


def parse_camodocal_yaml(text):
    """set_camera's keywords from the calibration text the reference's readFromYamlFile reads: `%YAML:1.0`, model_type, image_width,
    image_height and the model's parameter sections (distortion_parameters, projection_parameters, mirror_parameters,
    poly_parameters, affine_parameters; inv_poly_parameters is parse_camodocal_inv_poly's).  Only `key: value` lines are understood: a section is a key
    without a value followed by indented keys.  Everything else of the file (topics, extrinsics, matrices) is ignored."""
    top, sections, cur = {}, {}, None
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].rstrip()
        if not line.strip() or line.lstrip().startswith("%") or line.strip() == "---" or ":" not in line:
            continue
        key, val = line.split(":", 1)
        indented = key[:1] in " \t"
        key, val = key.strip(), val.strip().strip('"')
        if not indented:
            cur = None
            if val == "":
                cur = sections.setdefault(key, {})
            else:
                top[key] = val
        elif cur is not None:
            cur[key] = val
    name = top.get("model_type", "").upper()
    if name not in MODEL_NAMES:
        raise ValueError("model_type %r is not one of %s" % (top.get("model_type"), ", ".join(sorted(MODEL_NAMES))))
    model = MODEL_NAMES[name]
    out = dict(model=model, width=int(top["image_width"]), height=int(top["image_height"]))
    sec = lambda s: {k: float(v) for k, v in sections.get(s, {}).items()}
    if model == MODEL_PINHOLE:
        out.update({k: sec("distortion_parameters")[k] for k in ("k1", "k2", "p1", "p2")})
        out.update({k: sec("projection_parameters")[k] for k in ("fx", "fy", "cx", "cy")})
    elif model == MODEL_MEI:
        out["xi"] = sec("mirror_parameters")["xi"]
        out.update({k: sec("distortion_parameters")[k] for k in ("k1", "k2", "p1", "p2")})
        out.update({k: sec("projection_parameters")[k] for k in ("gamma1", "gamma2", "u0", "v0")})
    elif model == MODEL_SCARAMUZZA:
        out.update({"poly%d" % i: sec("poly_parameters")["p%d" % i] for i in range(5)})
        out.update({k: sec("affine_parameters")[k] for k in ("ac", "ad", "ae", "cx", "cy")})
    else:
        out.update({k: sec("projection_parameters")[k] for k in ("k2", "k3", "k4", "k5", "mu", "mv", "u0", "v0")})
    return out


def parse_camodocal_inv_poly(text):
    """SCARAMUZZA's inv_poly_parameters (p0, p1, ...) of the calibration text parse_camodocal_yaml reads, as a list of floats, lowest
    power first, for CameraHandle.set_inv_poly; [] where the text has no such section.  A function of its own: parse_camodocal_yaml's
    dict is set_camera's keywords and nothing else."""
    sec, inside = {}, False
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].rstrip()
        if not line.strip() or line.lstrip().startswith("%") or line.strip() == "---" or ":" not in line:
            continue
        key, val = line.split(":", 1)
        if key[:1] not in " \t":
            inside = key.strip() == "inv_poly_parameters" and val.strip() == ""
        elif inside:
            sec[key.strip()] = float(val.strip().strip('"'))
    out = []
    while "p%d" % len(out) in sec:
        out.append(sec["p%d" % len(out)])
    if len(out) != len(sec):
        raise ValueError("inv_poly_parameters must be p0, p1, ... without a gap")
    return out


class CameraLib:
    """libvio_camera_hip.so: vio_camera_*."""

    SYMBOLS = ["create", "destroy", "last_error", "version", "set", "set_config", "lift_batch", "undistort_batch", "reject_batch", "timing"]
    PROJECT_SYMBOLS = ["set_inv_poly", "project_batch"]                                    # include/vio_camera_project.h

    def __init__(self, path):
        from .capi import open_lib
        self.path = path
        self.dll, self.fn = open_lib(path, "vio_camera_", self.SYMBOLS)
        self.fn["create"].argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["set"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self.fn["set_config"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn["lift_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["undistort_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self.fn["reject_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn["timing"].argtypes = [C.c_void_p, C.c_void_p]
        self.fn.update(open_lib(path, "vio_camera_", self.PROJECT_SYMBOLS)[1])
        self.fn["set_inv_poly"].argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        self.fn["project_batch"].argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]

    def create(self, device=0, stream=None):
        """A vio_camera handle on `device`; stream: a hipStream_t (int) to enqueue on, or None for one of the library's own."""
        return CameraHandle(self, device, stream)


class CameraHandle(CompanionHandle):
    PREFIX = "vio_camera_"

    def __init__(self, lib, device=0, stream=None):
        self.lib = lib
        self.slot = 0
        self.h = C.c_void_p()
        st = lib.fn["create"](C.c_int32(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            raise VioError(st, "vio_camera_create")

    def _ck(self, st, where, allow_not_finite=False):
        if not (allow_not_finite and st == NOT_FINITE):
            super()._ck(st, where)

    def bind(self, slot):
        """A view of this handle whose .reject / .undistort / .lift use camera slot `slot` (the handle stays this one's to close)."""
        return _SlotView(self, int(slot))

    def set_camera(self, slot=0, model=MODEL_PINHOLE, width=752, height=480, **params):
        """Sets camera slot `slot`; params: the model's keywords (see PARAMS)."""
        p = model_params(int(model), **params)
        cam = VioCameraModel(int(model), int(width), int(height), 0, (C.c_double * MAX_PARAMS)(*(p + [0.0] * (MAX_PARAMS - len(p)))))
        self._ck(self.lib.fn["set"](self.h, C.c_int32(int(slot)), C.byref(cam)), "set")

    def set_config(self, seed=0, ransac_hypotheses=DEFAULT_HYPOTHESES, f_threshold=DEFAULT_F_THRESHOLD, focal_length=DEFAULT_FOCAL_LENGTH):
        cfg = VioRejectConfig(int(seed) & 0xFFFFFFFF, int(ransac_hypotheses), float(f_threshold), float(focal_length))
        self._ck(self.lib.fn["set_config"](self.h, C.byref(cfg)), "set_config")

    def lift_batch(self, items, angles=True):
        """liftProjective of every item: a list of dicts status, n_clamped, rays (n, 3) float64, angles (n, 2) float64 (theta, phi)."""
        B = len(items)
        arr = (VioCameraLiftItem * max(B, 1))()
        keep, outs = [], []
        for i, it in enumerate(items):
            p = _pts(it["pts"])
            rays = np.zeros((max(len(p), 1), 3), dtype=np.float64)
            ang = np.zeros((max(len(p), 1), 2), dtype=np.float64)
            keep.append(p)
            outs.append((rays, ang, len(p)))
            arr[i] = VioCameraLiftItem(len(p), int(it.get("slot", self.slot)), p.ctypes.data, rays.ctypes.data, ang.ctypes.data if angles else None)
        res = (VioCameraLiftResult * max(B, 1))()
        st = self.lib.fn["lift_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res))
        self._ck(st, "lift_batch", allow_not_finite=True)
        return [dict(status=int(res[i].status), n_clamped=int(res[i].n_clamped), rays=r[:n], angles=a[:n]) for i, (r, a, n) in enumerate(outs)]

    def lift(self, pts, slot=None):
        """The rays of one point set: (n, 3) float64."""
        return self.lift_batch([dict(pts=pts, slot=self.slot if slot is None else slot)])[0]["rays"]

    def undistort_batch(self, items):
        """undistortedPoints of every item: a list of dicts status, n_clamped, un_pts (n, 2) float32, velocity (n, 2) float32."""
        B = len(items)
        arr = (VioCameraUndistortItem * max(B, 1))()
        keep, outs = [], []
        for i, it in enumerate(items):
            p, ids = _pts(it["pts"]), _ids(it.get("ids"))
            pi, pu = _ids(it.get("prev_ids")), _pts(it.get("prev_un_pts"))
            if len(ids) != len(p) or len(pi) != len(pu):
                raise ValueError("item %d: ids needs one entry per point, prev_ids one per previous point" % i)
            un = np.full((max(len(p), 1), 2), np.nan, dtype=np.float32)
            vel = np.full((max(len(p), 1), 2), np.nan, dtype=np.float32)
            keep += [p, ids, pi, pu]
            outs.append((un, vel, len(p)))
            dt = it.get("dt")
            arr[i] = VioCameraUndistortItem(len(p), len(pi), p.ctypes.data, ids.ctypes.data, pi.ctypes.data, pu.ctypes.data,
                                            float(0.0 if dt is None else dt), un.ctypes.data, vel.ctypes.data, int(it.get("slot", self.slot)), 0)
        res = (VioCameraLiftResult * max(B, 1))()
        st = self.lib.fn["undistort_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res))
        self._ck(st, "undistort_batch", allow_not_finite=True)
        return [dict(status=int(res[i].status), n_clamped=int(res[i].n_clamped), un_pts=un[:n].copy(), velocity=vel[:n].copy())
                for i, (un, vel, n) in enumerate(outs)]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        """(un_pts, velocity) of one point set on the default slot (FeatureTracker's rejecter interface)."""
        if ids is None:
            ids = np.full(len(_pts(pts)), -1, dtype=np.int64)
        o = self.undistort_batch([dict(pts=pts, ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un_pts, dt=dt)])[0]
        return o["un_pts"], o["velocity"]

    def reject_batch(self, items):
        """rejectWithF of every pair: a list of dicts status, hyp, n_inliers, F (3, 3), mask (n,) bool."""
        B = len(items)
        arr = (VioCameraRejectItem * max(B, 1))()
        keep = []
        for i, it in enumerate(items):
            a, b = _pts(it["cur_pts"]), _pts(it["forw_pts"])
            if len(a) != len(b):
                raise ValueError("item %d: cur_pts and forw_pts must have one length" % i)
            keep += [a, b]
            arr[i] = VioCameraRejectItem(len(a), int(it.get("pair", 0)) & 0xFFFFFFFF, a.ctypes.data, b.ctypes.data, int(it.get("slot", self.slot)), 0)
        total = sum(int(arr[i].n) for i in range(B))
        mask = np.zeros(max(total, 1), dtype=np.uint8)
        res = (VioRejectResult * max(B, 1))()
        st = self.lib.fn["reject_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res), mask.ctypes.data)
        self._ck(st, "reject_batch", allow_not_finite=True)
        out, o = [], 0
        for i in range(B):
            r, n = res[i], int(arr[i].n)
            out.append(dict(status=int(r.status), hyp=int(r.hyp), n_inliers=int(r.n_inliers), F=np.array(r.F, dtype=np.float64).reshape(3, 3),
                            mask=mask[o:o + n].astype(bool)))
            o += n
        return out

    def reject(self, cur_pts, forw_pts, pair=0):
        """The pairs to keep on the default slot: (n,) bool (FeatureTracker's rejecter interface)."""
        return self.reject_batch([dict(cur_pts=cur_pts, forw_pts=forw_pts, pair=pair)])[0]["mask"]

    def set_inv_poly(self, slot, coeffs):
        """SCARAMUZZA's inv_poly_parameters of camera slot `slot`: 1 to INV_POLY_MAX finite coefficients, lowest power first.  The slot
        must hold a SCARAMUZZA camera; a later set_camera on it clears them."""
        c = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1)
        self._ck(self.lib.fn["set_inv_poly"](self.h, C.c_int32(int(slot)), C.c_int32(len(c)), c.ctypes.data if len(c) else None), "set_inv_poly")

    def project_batch(self, items):
        """spaceToPlane of every item (points (n, 3) float64 in the camera frame, slot): a list of dicts status, n_flagged, pixels (n, 2)
        float64, flags (n,) uint8 (0: usable; PROJECT_NOT_FINITE, PROJECT_BEHIND).  A point that is not finite gives its item
        NOT_FINITE and does not raise."""
        B = len(items)
        arr = (VioCameraProjectItem * max(B, 1))()
        keep, outs = [], []
        for i, it in enumerate(items):
            p = np.ascontiguousarray(it["points"], dtype=np.float64).reshape(-1, 3)
            pix = np.zeros((max(len(p), 1), 2), dtype=np.float64)
            fl = np.zeros(max(len(p), 1), dtype=np.uint8)
            keep.append(p)
            outs.append((pix, fl, len(p)))
            arr[i] = VioCameraProjectItem(len(p), int(it.get("slot", self.slot)), p.ctypes.data, pix.ctypes.data, fl.ctypes.data)
        res = (VioCameraProjectResult * max(B, 1))()
        st = self.lib.fn["project_batch"](self.h, C.c_int32(B), C.addressof(arr), C.addressof(res))
        self._ck(st, "project_batch", allow_not_finite=True)
        return [dict(status=int(res[i].status), n_flagged=int(res[i].n_flagged), pixels=pix[:n], flags=fl[:n]) for i, (pix, fl, n) in enumerate(outs)]

    def project(self, points, slot=None):
        """The pixels of one point set: (n, 2) float64 (NaN where a point has no finite pixel)."""
        return self.project_batch([dict(points=points, slot=self.slot if slot is None else slot)])[0]["pixels"]

    def timing(self):
        """ms of the last call that launched: host packing + upload, the kernel, the whole call."""
        t = (C.c_double * 3)()
        self._ck(self.lib.fn["timing"](self.h, t), "timing")
        return {"upload_ms": t[0], "kernel_ms": t[1], "total_ms": t[2]}


class _SlotView:
    """CameraHandle.bind(slot): the rejecter interface of the handle on another camera slot."""

    def __init__(self, handle, slot):
        self.handle, self.slot = handle, slot

    def reject(self, cur_pts, forw_pts, pair=0):
        return self.handle.reject_batch([dict(cur_pts=cur_pts, forw_pts=forw_pts, pair=pair, slot=self.slot)])[0]["mask"]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        if ids is None:
            ids = np.full(len(_pts(pts)), -1, dtype=np.int64)
        o = self.handle.undistort_batch([dict(pts=pts, ids=ids, prev_ids=prev_ids, prev_un_pts=prev_un_pts, dt=dt, slot=self.slot)])[0]
        return o["un_pts"], o["velocity"]

    def lift(self, pts):
        return self.handle.lift(pts, slot=self.slot)
