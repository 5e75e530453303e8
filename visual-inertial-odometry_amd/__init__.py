"""MI355X-native sliding-window VIO backend: host-side Python surface.

The product path is `csrc/libvio_hip.so` (hand-written HIP for gfx950 behind the C ABI of
include/vio_backend.h).  There is no CPU fallback: `load_hip()` raises if the library is missing.
"""
import os

from . import aif, batch_stream, camera, capi, clahe, covariance, detect, est, exrot, flow, fm, frame, frontend, imu, init, marg, pnp, reject, residuals, sfm, sharded, stream, synth
from .capi import (CAM_DIM, LOSS_CAUCHY, LOSS_HUBER, LOSS_TRIVIAL, LOSS_TUKEY, MARG_OLD, MARG_SECOND_NEW,
                   NUM_FRAMES, POSE_DIM, PRIOR_DIM, WINDOW_SIZE, VioConfig, VioContext, VioError, VioLib,
                   VioPreint, VioSolveReport)
from .aif import AifHandle, AifLib, BatchImageFrames, initialize_from_frames
from .camera import CameraHandle, CameraLib, parse_camodocal_yaml
from .clahe import ClaheHandle, ClaheLib
from .covariance import GAUGE_FIX_OLDEST, GAUGE_NONE, CovLib, pose_block, speed_bias_block
from .detect import DetectHandle, DetectLib
from .est import BatchEstimatorState, EstHandle, EstLib
from .exrot import ExrotHandle, ExrotLib
from .flow import FlowHandle, FlowLib
from .fm import BatchFeatureManager, FmHandle, FmLib
from .frame import FrameHandle, FrameLib
from .frontend import BatchFeatureTracker, FeatureTracker
from .imu import ImuHandle, ImuLib
from .init import InitHandle, InitLib
from .marg import MargHandle, MargLib
from .pnp import PnpHandle, PnpLib, all_frames_to_init_items, pnp_items_from_sfm
from .reject import RejectHandle, RejectLib
from .sfm import SfmHandle, SfmLib, sfm_items_to_init_items
from .residuals import FLAG_DEPTH, FLAG_REPROJ, FLAG_STATE, FLAGS_ALL, ResLib

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.environ.get("VIO_HIP_LIB") or os.path.join(PKG_DIR, "csrc", "libvio_hip.so")     # (VIO_HIP_LIB: another build, for A/B measurements)

COV_LIB = os.path.join(PKG_DIR, "csrc", "libvio_cov_hip.so")     # include/vio_covariance.h, linked against libvio_hip.so
RES_LIB = os.path.join(PKG_DIR, "csrc", "libvio_res_hip.so")     # include/vio_residuals.h, linked against libvio_hip.so
IMU_LIB = os.path.join(PKG_DIR, "csrc", "libvio_imu_hip.so")     # include/vio_imu.h, linked against libvio_hip.so
MARG_LIB = os.path.join(PKG_DIR, "csrc", "libvio_marg_hip.so")   # include/vio_marg.h, linked against libvio_hip.so
INIT_LIB = os.path.join(PKG_DIR, "csrc", "libvio_init_hip.so")   # include/vio_init.h, linked against libvio_hip.so
SFM_LIB = os.path.join(PKG_DIR, "csrc", "libvio_sfm_hip.so")     # include/vio_sfm.h; calls nothing of libvio_hip.so (linked like the others)
EXROT_LIB = os.path.join(PKG_DIR, "csrc", "libvio_exrot_hip.so")     # include/vio_exrot.h; calls nothing of libvio_hip.so either
PNP_LIB = os.path.join(PKG_DIR, "csrc", "libvio_pnp_hip.so")     # include/vio_pnp.h; calls nothing of libvio_hip.so either
FLOW_LIB = os.path.join(PKG_DIR, "csrc", "libvio_flow_hip.so")   # include/vio_flow.h; calls nothing of libvio_hip.so either
DETECT_LIB = os.path.join(PKG_DIR, "csrc", "libvio_detect_hip.so")   # include/vio_detect.h; calls nothing of libvio_hip.so either

REJECT_LIB = os.path.join(PKG_DIR, "csrc", "libvio_reject_hip.so")   # include/vio_reject.h; calls nothing of libvio_hip.so either
CLAHE_LIB = os.path.join(PKG_DIR, "csrc", "libvio_clahe_hip.so")     # include/vio_clahe.h; calls nothing of libvio_hip.so either
FRAME_LIB = os.path.join(PKG_DIR, "csrc", "libvio_frame_hip.so")     # include/vio_frame.h; calls nothing of libvio_hip.so either
FM_LIB = os.path.join(PKG_DIR, "csrc", "libvio_fm_hip.so")           # include/vio_fm.h; calls nothing of libvio_hip.so either
CAMERA_LIB = os.path.join(PKG_DIR, "csrc", "libvio_camera_hip.so")   # include/vio_camera.h; calls nothing of libvio_hip.so either
EST_LIB = os.path.join(PKG_DIR, "csrc", "libvio_est_hip.so")         # include/vio_est.h; calls nothing of libvio_hip.so either
AIF_LIB = os.path.join(PKG_DIR, "csrc", "libvio_aif_hip.so")         # include/vio_aif.h; calls nothing of libvio_hip.so either

_hip = None


def load_hip():
    """Load the HIP product library.  Raises (never falls back) when it has not been built."""
    global _hip
    if _hip is None:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64.  If this library were
        # loaded first it would pull in /opt/rocm's copies, and a later `import torch` would bring a second runtime
        # that finds no GPU (and RCCL would sit on the other one).  Importing torch first makes the dynamic loader
        # resolve our libamdhip64.so.7 to the copy torch already mapped.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip = VioLib(HIP_LIB, "vio_")
    return _hip


_hip_debug = None


def load_hip_debug():
    """The tests' build of the same sources with the diagnostic entry points (-DVIO_DEBUG_ENTRY_POINTS): csrc/diag/libvio_hip_debug.so."""
    global _hip_debug
    if _hip_debug is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip_debug = VioLib(os.environ.get("VIO_HIP_DEBUG_LIB") or os.path.join(PKG_DIR, "csrc", "diag", "libvio_hip_debug.so"), "vio_")
    return _hip_debug


_companions = {}


def _load_companion(key, cls, path):
    """A companion library, loaded once.  It resolves libvio_hip.so through its rpath: csrc/libvio_hip.so, which load_hip() loads
    first so that both share that one instance.  With VIO_HIP_LIB naming another build the process would hold two copies and hand
    one's contexts to the other, so that is refused."""
    if key not in _companions:
        own = os.path.join(PKG_DIR, "csrc", "libvio_hip.so")
        if os.path.realpath(HIP_LIB) != os.path.realpath(own):
            raise RuntimeError("load_%s: VIO_HIP_LIB=%s is not %s, the libvio_hip.so %s is linked against"
                               % (key, HIP_LIB, own, os.path.basename(path)))
        load_hip()
        _companions[key] = cls(path)
    return _companions[key]


def load_cov():
    """Load the covariance library (csrc/libvio_cov_hip.so)."""
    return _load_companion("cov", CovLib, COV_LIB)


def load_res():
    """Load the residual library (csrc/libvio_res_hip.so)."""
    return _load_companion("res", ResLib, RES_LIB)


def load_imu():
    """Load the IMU pre-integration library (csrc/libvio_imu_hip.so)."""
    return _load_companion("imu", ImuLib, IMU_LIB)


def load_marg():
    """Load the batched marginalisation library (csrc/libvio_marg_hip.so)."""
    return _load_companion("marg", MargLib, MARG_LIB)


def load_init():
    """Load the visual-inertial alignment library (csrc/libvio_init_hip.so)."""
    return _load_companion("init", InitLib, INIT_LIB)


def load_sfm():
    """Load the structure-from-motion library (csrc/libvio_sfm_hip.so)."""
    return _load_companion("sfm", SfmLib, SFM_LIB)


def load_exrot():
    """Load the extrinsic rotation calibration library (csrc/libvio_exrot_hip.so)."""
    return _load_companion("exrot", ExrotLib, EXROT_LIB)


def load_pnp():
    """Load the non-keyframe PnP library (csrc/libvio_pnp_hip.so)."""
    return _load_companion("pnp", PnpLib, PNP_LIB)


def load_flow():
    """Load the feature tracking library (csrc/libvio_flow_hip.so)."""
    return _load_companion("flow", FlowLib, FLOW_LIB)


def load_detect():
    """Load the corner detection library (csrc/libvio_detect_hip.so)."""
    return _load_companion("detect", DetectLib, DETECT_LIB)


def load_reject():
    """Load the outlier rejection and undistortion library (csrc/libvio_reject_hip.so)."""
    return _load_companion("reject", RejectLib, REJECT_LIB)


def load_clahe():
    """Load the CLAHE equalisation library (csrc/libvio_clahe_hip.so)."""
    return _load_companion("clahe", ClaheLib, CLAHE_LIB)


def load_frame():
    """Load the resident-frame library (csrc/libvio_frame_hip.so)."""
    return _load_companion("frame", FrameLib, FRAME_LIB)


def load_fm():
    """Load the batched FeatureManager library (csrc/libvio_fm_hip.so)."""
    return _load_companion("fm", FmLib, FM_LIB)


def load_est():
    """Load the batched Estimator state library (csrc/libvio_est_hip.so)."""
    return _load_companion("est", EstLib, EST_LIB)


def load_aif():
    """Load the resident all_image_frame library (csrc/libvio_aif_hip.so)."""
    return _load_companion("aif", AifLib, AIF_LIB)


def load_camera():
    """Load the camera model library (csrc/libvio_camera_hip.so)."""
    return _load_companion("camera", CameraLib, CAMERA_LIB)
