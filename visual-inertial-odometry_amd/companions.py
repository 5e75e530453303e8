"""The companion libraries, each declared once: plain data, read by the build (__graft_entry__.py, by path, without importing the
package) and by the loaders (__init__.py).

Key <key> names csrc/libvio_<key>_hip.so, linked from csrc/vio_<key>.o with the exports of csrc/libvio_<key>_hip.map and
against libvio_hip.so.  An entry holds what does not follow from the key:
    binding   "<module>.<class>" of the package: the ctypes class that opens the library
    what      the library in a few words (the docstring of load_<key>)
    source    the source file, where it is not vio_<key>.hip
    objects   objects of the product library's sources that it links besides its own
"""

LIB_NAME = "libvio_%s_hip"

COMPANIONS = {
    "cov": {"binding": "covariance.CovLib", "what": "covariance library", "source": "vio_covariance.hip"},
    "res": {"binding": "residuals.ResLib", "what": "residual library", "source": "vio_residuals.hip"},
    "imu": {"binding": "imu.ImuLib", "what": "IMU pre-integration library"},
    "marg": {"binding": "marg.MargLib", "what": "batched marginalisation library", "objects": ["host_dense"]},
    "init": {"binding": "init.InitLib", "what": "visual-inertial alignment library"},
    "sfm": {"binding": "sfm.SfmLib", "what": "structure-from-motion library"},
    "exrot": {"binding": "exrot.ExrotLib", "what": "extrinsic rotation calibration library"},
    "pnp": {"binding": "pnp.PnpLib", "what": "non-keyframe PnP library"},
    "flow": {"binding": "flow.FlowLib", "what": "feature tracking library"},
    "detect": {"binding": "detect.DetectLib", "what": "corner detection library"},
    "reject": {"binding": "reject.RejectLib", "what": "outlier rejection and undistortion library"},
    "clahe": {"binding": "clahe.ClaheLib", "what": "CLAHE equalisation library"},
    "frame": {"binding": "frame.FrameLib", "what": "resident-frame library"},
    "fm": {"binding": "fm.FmLib", "what": "batched FeatureManager library"},
    "camera": {"binding": "camera.CameraLib", "what": "camera model library"},
    "est": {"binding": "est.EstLib", "what": "batched Estimator state library"},
    "aif": {"binding": "aif.AifLib", "what": "resident all_image_frame library"},
}
