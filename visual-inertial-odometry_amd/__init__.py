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
from .companions import COMPANIONS, LIB_NAME
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


def _define_companion(key, entry):
    """vio.<KEY>_LIB, the library's path, and vio.load_<key>(), which loads it once with the binding class of its table entry."""
    module, cls = entry["binding"].split(".")
    cls = getattr(globals()[module], cls)
    path = os.path.join(PKG_DIR, "csrc", LIB_NAME % key + ".so")      # linked against csrc/libvio_hip.so

    def load():
        return _load_companion(key, cls, path)

    load.__name__ = load.__qualname__ = "load_" + key
    load.__doc__ = "Load the %s (csrc/%s)." % (entry["what"], os.path.basename(path))
    globals().update({key.upper() + "_LIB": path, load.__name__: load})


for _key, _entry in COMPANIONS.items():
    _define_companion(_key, _entry)
