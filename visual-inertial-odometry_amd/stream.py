"""Sliding-window stream driver over synthetic data.

Host-side control flow of `Estimator::processImage` -> `solveOdometry` -> `slideWindow` for a stream of frames, with
any library that exports the C ABI as the backend:

    per new frame:   predict its state from the last one with the pre-integrated IMU (processIMU,
                     VM/src/estimator.cpp:105-139), [f_manager.triangulate], vector2double (:505-547), Solve(10) with the
                     prior (problemSolve :902-1073), double2vector's yaw/position re-anchoring (:549-600), then
      keyframe       MargOldFrame (:693-829), slideWindowOld (:1187-1199): the oldest frame leaves; landmarks hosted
                     in it move to their next frame with the depth carried over (removeBackShiftDepth,
                     feature_manager.cpp:276-312) or die with it
      non-keyframe   MargNewFrame (:830-901), slideWindowNew (:1201-1206): the second-newest frame leaves, its
                     observations are dropped (removeFront, feature_manager.cpp:331-350), its IMU samples are appended
                     to the interval before it (pre_integrations[frame_count - 1]->push_back, :1163-1176)

Which frames are keyframes is the front-end's call (the parallax test of addFeatureCheckParallax); here it is a
parameter (`nonkey_every`).  Poses are written in TUM format (`stamp px py pz qx qy qz qw`, System.cpp:438) so that
`evo_ape tum` can be run on the output.
"""
import math

import numpy as np

from . import synth
from .imu import record_dict
from .capi import MARG_OLD, MARG_SECOND_NEW, NUM_FRAMES, WINDOW_SIZE


def r2ypr(R):
    """Utility::R2ypr (VM/include/utility/utility.h:68-84), degrees."""
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = math.atan2(n[1], n[0])
    p = math.atan2(-n[2], n[0] * math.cos(y) + n[1] * math.sin(y))
    r = math.atan2(a[0] * math.sin(y) - a[1] * math.cos(y), -o[0] * math.sin(y) + o[1] * math.cos(y))
    return np.array([y, p, r]) / math.pi * 180.0


def ypr2r(ypr):
    """Utility::ypr2R (utility.h:86-110), degrees."""
    y, p, r = (v / 180.0 * math.pi for v in ypr)
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    return Rz @ Ry @ Rx


def anchor_gauge(poses_before, poses_after, sb_after):
    """double2vector's re-anchoring of yaw and position to the pre-solve frame 0 (estimator.cpp:551-600)."""
    R0_before = synth.quat_to_rot(poses_before[0, 3:7])
    R0_after = synth.quat_to_rot(poses_after[0, 3:7])       # not normalised here (:557-561), normalised below (:579)
    o0, o00 = r2ypr(R0_before), r2ypr(R0_after)
    rot_diff = ypr2r([o0[0] - o00[0], 0, 0])
    if abs(abs(o0[1]) - 90) < 1.0 or abs(abs(o00[1]) - 90) < 1.0:
        rot_diff = R0_before @ R0_after.T
    poses, sb = poses_after.copy(), sb_after.copy()
    for i in range(NUM_FRAMES):
        q = poses_after[i, 3:7] / np.linalg.norm(poses_after[i, 3:7])
        poses[i, 3:7] = synth.rot_to_quat(rot_diff @ synth.quat_to_rot(q))
        poses[i, 0:3] = rot_diff @ (poses_after[i, 0:3] - poses_after[0, 0:3]) + poses_before[0, 0:3]
        sb[i, 0:3] = rot_diff @ sb_after[i, 0:3]
    return poses, sb


def visual_trajectory(stream, frames, l=0, scale=1.0, rot_noise=0.0, pos_noise=0.0, seed=0):
    """The SfM stand-in of the initialisation: ImageFrame::R / T of the global frames `frames` as initialStructure leaves them
    (estimator.cpp:224-382) — camera frame frames[l] is the origin, R = R_{c_l c_k} RIC^T (the body's rotation in c_l) and
    T = p_{c_l c_k} / scale (the camera centre, up to the unknown scale).  It replaces relativePose + GlobalSFM + solvePnP, which need
    OpenCV and Ceres.  rot_noise: std (rad) of a right-multiplied rotation per frame; pos_noise: std (m, metric) added to every camera
    centre before the division by scale.  Returns (R (F, 3, 3), T (F, 3))."""
    rng = np.random.RandomState(seed)
    ric = np.asarray(getattr(stream, "ric", synth.R_IC), dtype=np.float64)
    tic = np.asarray(getattr(stream, "tic", synth.T_IC), dtype=np.float64)
    fl = frames[l]
    Rcl = stream.R[fl] @ ric
    pcl = stream.P[fl] + stream.R[fl] @ tic
    R, T = np.zeros((len(frames), 3, 3)), np.zeros((len(frames), 3))
    for k, f in enumerate(frames):
        Rb = Rcl.T @ stream.R[f]
        if rot_noise:
            Rb = Rb @ _small_rot(rng.normal(0.0, rot_noise, 3))
        R[k] = Rb
        p = Rcl.T @ (stream.P[f] + stream.R[f] @ tic - pcl)
        if pos_noise:
            p = p + rng.normal(0.0, pos_noise, 3)
        T[k] = p / scale
    return R, T


def _small_rot(th):
    q = np.array([th[0] / 2, th[1] / 2, th[2] / 2, 1.0])
    return synth.quat_to_rot(q / np.linalg.norm(q))


class SyntheticStream:
    """Ground truth + measurements of `n_frames` keyframes on the simulator's trajectory."""

    def __init__(self, n_frames=30, landmarks_per_frame=30, track_len=5, seed=0, t0=1.0, frame_dt=0.1, imu_rate=200,
                 pixel_noise=1.0 / synth.FOCAL):
        rng = np.random.RandomState(seed)
        self.n_frames, self.frame_dt, self.t0 = n_frames, frame_dt, t0
        self.times = [t0 + frame_dt * k for k in range(n_frames)]
        gt = [synth.motion_model(t) for t in self.times]
        self.R = np.stack([m.Rwb for m in gt])
        self.P = np.stack([m.twb for m in gt])
        self.V = np.stack([m.vel for m in gt])
        self.Q = np.stack([synth.rot_to_quat(m.Rwb) for m in gt])
        self.ext = np.concatenate([synth.T_IC, synth.rot_to_quat(synth.R_IC)])
        n_sub = int(round(frame_dt * imu_rate))
        dt = frame_dt / n_sub
        self.preint, self.imu = [], []      # [k]: frame k -> k+1: pre-integration and the raw samples it was made of
        for k in range(n_frames - 1):
            ms = [synth.motion_model(self.times[k] + j * dt) for j in range(n_sub + 1)]
            self.imu.append(dict(acc0=ms[0].acc, gyr0=ms[0].gyro, dt=[dt] * n_sub, acc=[m.acc for m in ms[1:]],
                                 gyr=[m.gyro for m in ms[1:]]))
            self.preint.append(synth.preintegrate(ms[0].acc, ms[0].gyro, np.zeros(3), np.zeros(3), [dt] * n_sub,
                                                  [m.acc for m in ms[1:]], [m.gyro for m in ms[1:]]))
        make_tracks(self, rng, landmarks_per_frame, track_len, pixel_noise)


IMU_COLUMNS = ("timestamp", "q_w", "q_x", "q_y", "q_z", "p_x", "p_y", "p_z", "gyro_x", "gyro_y", "gyro_z", "acc_x", "acc_y", "acc_z")
KEYFRAME_COLUMNS = ("timestamp", "id", "x", "y", "z", "lambda", "x_normalized", "y_normalized", "u", "v")


def write_simulator_files(stream, out_dir, fx=synth.FOCAL, cx=255.0, cy=255.0):
    """Write a stream in the file formats of the reference's simulator: `imu_pose.txt`
    (timestamp, ground-truth q and p, gyro, acc: simulator/src/utilities.cpp:150-171; the runner reads timestamp, gyro
    and acc by name and ignores the rest, run_vio_simulation.cpp:43-49) and one `keyframe/all_points_<n>.txt` per frame
    (timestamp, id, world point, lambda, normalised point, pixel: utilities.cpp:37-63, read at
    run_vio_simulation.cpp:163-170).  Three extra columns v_x, v_y, v_z carry the ground-truth velocity."""
    import os
    os.makedirs(os.path.join(out_dir, "keyframe"), exist_ok=True)
    st = stream
    with open(os.path.join(out_dir, "imu_pose.txt"), "w") as f:
        f.write(",".join(IMU_COLUMNS + ("v_x", "v_y", "v_z")) + "\n")
        rows = []
        for k, iv in enumerate(st.imu):
            t = st.times[k]
            if k == 0:
                rows.append((t, iv["gyr0"], iv["acc0"]))
            for dt, a, g in zip(iv["dt"], iv["acc"], iv["gyr"]):
                t = t + dt
                rows.append((t, g, a))
            rows[-1] = (st.times[k + 1], rows[-1][1], rows[-1][2])      # the frame stamp itself, not an accumulated sum
        for t, g, a in rows:
            m = synth.motion_model(t)
            q = synth.rot_to_quat(m.Rwb)                                 # (x, y, z, w)
            vals = [t, q[3], q[0], q[1], q[2], *m.twb, *g, *a, *m.vel]
            f.write(",".join(repr(float(v)) for v in vals) + "\n")
    for k in range(st.n_frames):
        with open(os.path.join(out_dir, "keyframe", "all_points_%d.txt" % k), "w") as f:
            f.write(",".join(KEYFRAME_COLUMNS) + "\n")
            for l, h in enumerate(st.lm_host):
                if h == k:
                    xy = np.asarray(st.lm_px[l], dtype=np.float64)
                elif k in st.lm_obs[l]:
                    xy = np.asarray(st.lm_obs[l][k], dtype=np.float64)
                else:
                    continue
                pw = st.R[h] @ (synth.R_IC @ (np.array([st.lm_px[l][0], st.lm_px[l][1], 1.0]) * st.lm_depth[l]) + synth.T_IC) + st.P[h]
                vals = [st.times[k], l, *pw, 1.0, xy[0], xy[1], fx * xy[0] + cx, fx * xy[1] + cy]
                f.write(",".join(str(v) if isinstance(v, int) else repr(float(v)) for v in vals) + "\n")


def _read_csv(path, wanted, optional=()):
    """Columns by name, extra columns ignored (io::ignore_extra_column of the reference's CSV reader)."""
    with open(path) as f:
        header = [h.strip() for h in f.readline().strip().split(",")]
        missing = [w for w in wanted if w not in header]
        if missing:
            raise ValueError("%s: missing column(s) %s" % (path, ", ".join(missing)))
        cols = [header.index(w) for w in wanted]
        opt = [header.index(w) if w in header else -1 for w in optional]
        data, extra = [], []
        for line in f:
            line = line.strip()
            if not line:
                continue
            parts = line.split(",")
            data.append([float(parts[c]) for c in cols])
            extra.append([float(parts[c]) if c >= 0 else np.nan for c in opt])
    return np.array(data, dtype=np.float64).reshape(-1, len(wanted)), np.array(extra, dtype=np.float64).reshape(-1, len(optional))


def cut_imu_intervals(t_imu, meas, times, noise=None):
    """IMU samples (stamps t_imu, rows acc | gyro) cut into per-frame intervals the way System::ProcessBackEnd does
    (System.cpp:363-401): every sample up to the image stamp, then one sample linearly interpolated to the stamp itself, which also
    opens the next interval (Estimator::processIMU: acc_0 / gyr_0).  Returns (raw intervals, their pre-integrations at zero bias)."""
    def at(t):
        j = int(np.clip(np.searchsorted(t_imu, t), 1, len(t_imu) - 1))
        w = (t - t_imu[j - 1]) / (t_imu[j] - t_imu[j - 1])
        w = min(max(w, 0.0), 1.0)
        return (1.0 - w) * meas[j - 1] + w * meas[j]

    ivs, pres = [], []
    for k in range(len(times) - 1):
        ta, tb = times[k], times[k + 1]
        first = at(ta)
        dts, accs, gyrs, cur = [], [], [], ta
        for j in np.nonzero((t_imu > ta) & (t_imu <= tb))[0]:
            if t_imu[j] - cur > 0:
                dts.append(float(t_imu[j] - cur)); accs.append(meas[j, 0:3].copy()); gyrs.append(meas[j, 3:6].copy())
                cur = float(t_imu[j])
        if tb - cur > 1e-12:
            last = at(tb)
            dts.append(float(tb - cur)); accs.append(last[0:3].copy()); gyrs.append(last[3:6].copy())
        ivs.append(dict(acc0=first[0:3].copy(), gyr0=first[3:6].copy(), dt=dts, acc=accs, gyr=gyrs))
        pres.append(synth.preintegrate(first[0:3], first[3:6], np.zeros(3), np.zeros(3), dts, accs, gyrs, **(noise or {})))
    return ivs, pres


def make_tracks(st, rng, landmarks_per_frame, track_len, pixel_noise, ric=None, tic=None):
    """Synthetic vision on a stream's ground-truth poses: landmarks hosted in frame h, seen in h+1 .. h+track_len."""
    ric = synth.R_IC if ric is None else ric
    tic = synth.T_IC if tic is None else tic
    st.lm_host, st.lm_px, st.lm_depth, st.lm_obs = [], [], [], []
    for h in range(st.n_frames - 1):
        for _ in range(landmarks_per_frame):
            px = rng.uniform(-0.5, 0.5, 2)
            depth = rng.uniform(4.0, 10.0)
            pw = st.R[h] @ (ric @ (np.array([px[0], px[1], 1.0]) * depth) + tic) + st.P[h]
            obs = {}
            for j in range(h + 1, min(h + 1 + track_len, st.n_frames)):
                pc = ric.T @ (st.R[j].T @ (pw - st.P[j]) - tic)
                pc[2] = max(pc[2], 0.5)
                obs[j] = pc[0:2] / pc[2] + rng.normal(0.0, pixel_noise, 2)
            st.lm_host.append(h)
            st.lm_px.append(px)
            st.lm_depth.append(depth)
            st.lm_obs.append(obs)
    st.init_noise = rng.normal(size=(len(st.lm_host),))


class RealImuStream:
    """Real inertial data, synthetic vision: the nearest runnable stand-in for the reference's EuRoC runs (VM/test/run_euroc.cpp:26-110
    feeds MH_05_imu0.txt and the images of MH_05_cam0.txt; the images and the OpenCV front-end are not in the tree, the IMU file
    and the stamps are).  `data` = tests/golden/mh05_imu_stretch.npz: the samples are cut at the frame stamps as System::ProcessBackEnd
    does and pre-integrated with the noise parameters of euroc_config.yaml; the "ground truth" is the trajectory those
    pre-integrations define from a gravity-aligned start at rest (P_j = P_i + V_i dt - g dt^2 / 2 + R_i delta_p, ...: the IMU
    factors' own model, integration_base.h:160-186, so the inertial residuals vanish on it), and the landmarks are drawn in front of
    its camera poses with the sequence's extrinsic.  Same attributes as SyntheticStream: StreamDriver runs on it."""

    def __init__(self, data, n_frames=None, landmarks_per_frame=30, track_len=5, seed=0, pixel_noise=1.0 / 460.0):
        rng = np.random.RandomState(seed)
        cam_t = np.asarray(data["cam_t"], dtype=np.float64)
        self.n_frames = int(n_frames or len(cam_t))
        self.times = [float(t) for t in cam_t[:self.n_frames]]
        self.t0, self.frame_dt = self.times[0], (self.times[-1] - self.times[0]) / max(1, self.n_frames - 1)
        self.noise = dict(acc_n=float(data["acc_n"]), gyr_n=float(data["gyr_n"]), acc_w=float(data["acc_w"]), gyr_w=float(data["gyr_w"]))
        self.g_norm = float(data["g_norm"])
        self.ric, self.tic = np.asarray(data["ric"], dtype=np.float64), np.asarray(data["tic"], dtype=np.float64)
        self.ext = np.concatenate([self.tic, synth.rot_to_quat(self.ric)])
        meas = np.concatenate([np.asarray(data["imu_acc"]), np.asarray(data["imu_gyr"])], axis=1)
        self.imu, self.preint = cut_imu_intervals(np.asarray(data["imu_t"], dtype=np.float64), meas, self.times, self.noise)
        # start: at rest, the first accelerometer sample straight up (R_0 a_0 || +z: the specific force of a body at rest is -g)
        a0 = self.imu[0]["acc0"] / np.linalg.norm(self.imu[0]["acc0"])
        z = np.array([0.0, 0.0, 1.0])
        v = np.cross(a0, z)
        c = float(a0 @ z)
        K = synth.skew(v)
        R0 = np.eye(3) + K + K @ K / (1.0 + c)
        g = np.array([0.0, 0.0, self.g_norm])
        self.R, self.P, self.V = np.zeros((self.n_frames, 3, 3)), np.zeros((self.n_frames, 3)), np.zeros((self.n_frames, 3))
        self.Q = np.zeros((self.n_frames, 4))
        self.R[0], self.Q[0] = R0, synth.rot_to_quat(R0)
        for k, pre in enumerate(self.preint):
            dt = pre["sum_dt"]
            self.P[k + 1] = self.P[k] + self.V[k] * dt - 0.5 * g * dt * dt + self.R[k] @ pre["delta_p"]
            self.V[k + 1] = self.V[k] - g * dt + self.R[k] @ pre["delta_v"]
            q = synth.quat_mul(self.Q[k], pre["delta_q"])
            self.Q[k + 1] = q / np.linalg.norm(q)
            self.R[k + 1] = synth.quat_to_rot(self.Q[k + 1])
        self.has_ground_truth = True
        make_tracks(self, rng, landmarks_per_frame, track_len, pixel_noise, self.ric, self.tic)


class SimulatorFileStream:
    """A stream read from the reference simulator's files (see write_simulator_files): the same attributes as
    SyntheticStream, so StreamDriver runs on either.  IMU samples are cut into per-frame intervals the way
    System::ProcessBackEnd does (System.cpp:363-401): every sample up to the image stamp, then one sample linearly
    interpolated to the stamp itself, which also opens the next interval (Estimator::processIMU, acc_0 / gyr_0)."""

    def __init__(self, directory, imu_file="imu_pose.txt", keyframe_dir="keyframe", max_frames=None, seed=0):
        import os
        import re
        imu, extra = _read_csv(os.path.join(directory, imu_file),
                               ("timestamp", "gyro_x", "gyro_y", "gyro_z", "acc_x", "acc_y", "acc_z"),
                               ("q_w", "q_x", "q_y", "q_z", "p_x", "p_y", "p_z", "v_x", "v_y", "v_z"))
        files = []
        for name in os.listdir(os.path.join(directory, keyframe_dir)):
            m = re.fullmatch(r"all_points_(.*)\.txt", name)
            if m:
                files.append((int(m.group(1)), os.path.join(directory, keyframe_dir, name)))
        files.sort()                                        # by sequence id, run_vio_simulation.cpp:141-147
        if max_frames:
            files = files[:max_frames]
        frames = []
        for _, path in files:
            kf, world = _read_csv(path, ("timestamp", "id", "x_normalized", "y_normalized"), ("x", "y", "z"))
            if len(kf):
                frames.append((kf, world))
        self.n_frames = len(frames)
        self.times = [float(kf[0, 0]) for kf, _ in frames]
        self.t0, self.frame_dt = self.times[0], (self.times[-1] - self.times[0]) / max(1, self.n_frames - 1)
        self.ext = np.concatenate([synth.T_IC, synth.rot_to_quat(synth.R_IC)])
        t_imu = imu[:, 0]

        def at(t, cols):                                    # linear interpolation of imu/extra columns at stamp t
            j = int(np.clip(np.searchsorted(t_imu, t), 1, len(t_imu) - 1))
            w = (t - t_imu[j - 1]) / (t_imu[j] - t_imu[j - 1])
            w = min(max(w, 0.0), 1.0)
            return (1.0 - w) * cols[j - 1] + w * cols[j]

        # ground truth at the frame stamps (initial guesses and the ATE reference); velocity by central differences
        # of the position when the file has no v columns
        have_gt = not np.isnan(extra[:, 0:7]).any()
        self.P, self.Q, self.R, self.V = (np.zeros((self.n_frames, 3)), np.zeros((self.n_frames, 4)),
                                          np.zeros((self.n_frames, 3, 3)), np.zeros((self.n_frames, 3)))
        for k, t in enumerate(self.times):
            if not have_gt:
                self.Q[k] = (0, 0, 0, 1)
                self.R[k] = np.eye(3)
                continue
            g = at(t, extra)
            q = np.array([g[1], g[2], g[3], g[0]])
            self.Q[k] = q / np.linalg.norm(q)
            self.R[k] = synth.quat_to_rot(self.Q[k])
            self.P[k] = g[4:7]
            if not np.isnan(extra[:, 7:10]).any():
                self.V[k] = g[7:10]
            else:
                h = 2.0 * np.median(np.diff(t_imu))
                self.V[k] = (at(t + h, extra)[4:7] - at(t - h, extra)[4:7]) / (2.0 * h)
        self.has_ground_truth = bool(have_gt)
        # IMU intervals
        meas = imu[:, [4, 5, 6, 1, 2, 3]]                  # acc, gyro
        self.imu, self.preint = cut_imu_intervals(t_imu, meas, self.times)
        # tracks: a feature id is hosted by the first frame that sees it
        index = {}
        self.lm_host, self.lm_px, self.lm_depth, self.lm_obs, self.lm_id = [], [], [], [], []
        for k, (kf, world) in enumerate(frames):
            for row, pw in zip(kf, world):
                fid = int(row[1])
                if fid not in index:
                    index[fid] = len(self.lm_host)
                    self.lm_host.append(k)
                    self.lm_px.append(row[2:4].copy())
                    depth = np.nan
                    if have_gt and not np.isnan(pw).any():
                        pc = synth.R_IC.T @ (self.R[k].T @ (pw - self.P[k]) - synth.T_IC)
                        depth = float(pc[2])
                    self.lm_depth.append(depth)
                    self.lm_obs.append({})
                    self.lm_id.append(fid)
                else:
                    self.lm_obs[index[fid]][k] = row[2:4].copy()
        self.init_noise = np.random.RandomState(seed).normal(size=(len(self.lm_host),))


def aif_flush(drivers):
    """Feeds the INITIAL-state steps that `drivers` (all on one aif.AifHandle) have queued into their all_image_frame slots: per step
    one slide_batch, one imu_batch and one image_batch over every driver that has one.  A refused item (POOL_FULL, FRAMES_FULL,
    NO_FRAME) would leave its slot out of step with the driver's lists, so it raises."""
    def check(d, name, r):
        if r["status"] != 0:
            raise RuntimeError("StreamDriver: vio_aif_%s refused slot %d with status %d" % (name, d.aif_slot, r["status"]))
    _flush(drivers, "aif", check)


def est_flush(drivers):
    """Feeds the INITIAL-state steps that `drivers` (all on one est.EstHandle, initialize=dict(state=)) have queued into their
    estimator-state slots, as aif_flush does for all_image_frame: per step one slide_batch (a failed try's slideWindow), one imu_batch
    (processIMU) and one image_batch (processImage) over every driver that has one.  A slot that did not follow (a window that is not
    full at a slide, POOL_FULL) would be out of step with its driver, so it raises."""
    def check(d, name, r):
        if r["status"] != 0 or (name == "slide_batch" and not r["slid"]):
            raise RuntimeError("StreamDriver: vio_est_%s did not serve slot %d (status %d, frame_count %d)" % (name, d.est_slot, r["status"], r["frame_count"]))
    _flush(drivers, "est", check)


def _flush(drivers, kind, check):
    """The queued (slide, imu, image) steps of `drivers` into their `kind` ("aif" or "est") slots, the oldest step of every driver
    first: one call per part over the drivers whose step has it; check(driver, method, result) raises where a slot did not follow."""
    queue, slot = "_%s_queue" % kind, "%s_slot" % kind
    todo = [d for d in drivers if getattr(d, queue)]
    while todo:
        steps = [(d, getattr(d, queue).pop(0)) for d in todo]
        for part, name in enumerate(("slide_batch", "imu_batch", "image_batch")):
            who = [(d, st[part]) for d, st in steps if st[part] is not None]
            if not who:
                continue
            res = getattr(getattr(who[0][0], kind), name)([(getattr(d, slot),) + item for d, item in who])
            for (d, _), r in zip(who, res):
                check(d, name, r)
        todo = [d for d in todo if getattr(d, queue)]


def est_init_apply(drivers, results):
    """visualInitialAlign's state change of every driver that initialised, in its slot: one init_apply_batch on each try's poses,
    speed_bias, g and rot (include/vio_est_init.h), with commit_last: the reference runs no failureDetection behind the first solve
    (estimator.cpp:192-201), update_batch always does, so last_P starts at the initialisation's newest frame and not at whatever the
    slot held."""
    res = drivers[0].est.init_apply_batch([(d.est_slot, np.asarray(r["poses"], dtype=np.float64).reshape(NUM_FRAMES, 7),
                                            np.asarray(r["speed_bias"], dtype=np.float64).reshape(NUM_FRAMES, 9), r["g"], r["rot"], True)
                                           for d, r in zip(drivers, results)])
    for d, r in zip(drivers, res):
        if r["status"] != 0:
            raise RuntimeError("StreamDriver: vio_est_init_apply_batch refused slot %d with status %d (frame_count %d)" % (d.est_slot, r["status"], r["frame_count"]))


def est_relinearize(drivers):
    """repropagate in the slots of the drivers that ask for it (state=dict(relinearize=)): one relinearize_batch; each driver's count
    goes to its `repropagated`."""
    who = [d for d in drivers if d.est_relin is not None]
    if who:
        for d, r in zip(who, who[0].est.relinearize_batch([(d.est_slot,) + d.est_relin for d in who])):
            d.repropagated.append(int(r["n_relinearized"]))


def _parse_state(state):
    """(handle, slot, relinearize thresholds or None) of a state= argument: a tuple (handle, slot), or a dict(handle=, slot=,
    relinearize=(ba_thresh, bg_thresh))."""
    if isinstance(state, dict):
        relin = state.get("relinearize")
        return state["handle"], int(state["slot"]), None if relin is None else (float(relin[0]), float(relin[1]))
    return state[0], int(state[1]), None


# ---- the FeatureManager of `drivers` (all on one fm.FmHandle, features=) in one call each ------------------------
FM_DEPTH_SET, FM_BACK_SHIFT_DEPTH, FM_BACK, FM_FRONT = 0, 0, 1, 2        # include/vio_fm.h


def _fm_checked(drivers, res, what):
    """A slot the device refused is as it was and out of step with its driver, so it raises."""
    for d, r in zip(drivers, res):
        if r["status"] != 0:
            raise RuntimeError("StreamDriver: vio_fm_%s refused slot %d with status %d" % (what, d.fm_slot, r["status"]))
    return res


def fm_add(drivers, frames, frame_count=WINDOW_SIZE):
    """addFeatureCheckParallax of global frame frames[i] of every driver as window frame `frame_count`: one add_batch."""
    items = [(d.fm_slot, frame_count) + d.frame_points(f) for d, f in zip(drivers, frames)]
    for d, r in zip(drivers, _fm_checked(drivers, drivers[0].fm.add_batch(items), "add_batch")):
        d.fm_keyframe.append(int(r["keyframe"]))


def fm_windows(drivers, triangulate):
    """[f_manager.triangulate,] getDepthVector and the edge loop on every driver's current poses: one export_batch.  Per driver
    (Window, feature ids), what ensure_depths + window_arrays give."""
    res = _fm_checked(drivers, drivers[0].fm.export_batch([(d.fm_slot, d.poses, d.ext) for d in drivers], triangulate=triangulate), "export_batch")
    out = []
    for d, r in zip(drivers, res):
        d.n_triangulated += int(r["n_triangulated"])
        w = synth.Window(poses=d.poses.copy(), speed_bias=d.sb.copy(), ext=d.ext.copy(), inv_depth=r["inv_depth"], lm=r["lm"],
                         host=r["host"], target=r["target"], pts_i=r["pts_i"], pts_j=r["pts_j"], preint=list(d.preint), prior=d.prior,
                         n_landmarks=len(r["feature_ids"]), n_observations=len(r["lm"]))
        out.append((w, [int(l) for l in r["feature_ids"]]))
    return out


def fm_set_depths(drivers, inv_depths):
    """setDepth from every driver's solved inverse depths [and removeFailures]: one set_depth_batch per setting of the option."""
    for flag in (False, True):
        who = [(d, x) for d, x in zip(drivers, inv_depths) if d.fm_remove_failures == flag]
        if who:
            ds = [d for d, _ in who]
            _fm_checked(ds, ds[0].fm.set_depth_batch([(d.fm_slot, x) for d, x in who], FM_DEPTH_SET, flag), "set_depth_batch")


def fm_remove(drivers, ids_lists):
    """removeOutlier / removeFailures by feature id in every driver's slot: one remove_batch.  Each call's erased rows go to the
    driver's fm_erased."""
    res = _fm_checked(drivers, drivers[0].fm.remove_batch([(d.fm_slot, np.asarray(ids, dtype=np.int64).reshape(-1)) for d, ids in zip(drivers, ids_lists)]),
                      "remove_batch")
    for d, r in zip(drivers, res):
        d.fm_erased.append(int(r["n_rows"]))


def fm_slide(drivers, kinds, mats=None):
    """kinds[i]: FM_BACK_SHIFT_DEPTH with mats[i] = (marg_R, marg_P, new_R, new_P), FM_BACK, or FM_FRONT (frame_count WINDOW_SIZE): one
    slide_batch."""
    items = []
    for i, (d, k) in enumerate(zip(drivers, kinds)):
        items.append((d.fm_slot, k, WINDOW_SIZE) + (tuple(mats[i]) if k == FM_BACK_SHIFT_DEPTH else ()))
    _fm_checked(drivers, drivers[0].fm.slide_batch(items), "slide_batch")


def fm_tracks(drivers):
    """Every driver's list (sfm_f) in one tracks_batch."""
    return _fm_checked(drivers, drivers[0].fm.tracks_batch([d.fm_slot for d in drivers]), "tracks_batch")


def fm_init_depths(drivers, items, scales):
    """visualInitialAlign's depth hand-over of every driver that initialised: clearDepth, triangulate on items[i]'s SfM poses with
    tic = 0, estimated_depth *= scales[i] (estimator.cpp:406-442): one init_depth_batch."""
    args = [(d.fm_slot, sfm_poses(it), np.concatenate([np.zeros(3), d.ext[3:7]]), float(s)) for d, it, s in zip(drivers, items, scales)]
    for d, r in zip(drivers, _fm_checked(drivers, drivers[0].fm.init_depth_batch(args), "init_depth_batch")):
        d.n_triangulated += int(r["n_triangulated"])


def sfm_poses(item):
    """An alignment item's SfM poses (R, T) as the (NUM_FRAMES, 7) array a triangulation takes."""
    sfm = np.zeros((NUM_FRAMES, 7))
    sfm[:, 0:3] = item["T"]
    for i in range(NUM_FRAMES):
        sfm[i, 3:7] = synth.rot_to_quat(item["R"][i])
    return sfm


# ---- one frame and one INITIAL round of a group of drivers (a StreamDriver alone is a group of one) ---------------
class OwnContexts:
    """The frame's three heavy calls, each driver's on its own context: what StreamDriver.step issues.  (batch_stream.BatchedCalls
    issues them once for the group.)"""

    def solve(self, drivers):
        """Problem::Solve(10) of every loaded window; the reports."""
        return [d.ctx.solve(10) for d in drivers]

    def flags(self, drivers, windows):
        """The residual query's landmark flags on the solved states, per driver; None for a driver without outlier_px."""
        return [None if d.outlier_px is None else d.ctx.residuals(w, outlier_px=d.outlier_px)["flags"] for d, w in zip(drivers, windows)]

    def marginalize(self, drivers, jobs):
        """jobs[i] = (flag, re-anchored window, prior): the new priors, through vio_marginalize on the reloaded context."""
        out = []
        for d, (kind, w2, _) in zip(drivers, jobs):
            d.ctx.load(w2)
            out.append(d.ctx.marginalize(kind))
        return out


def step_group(drivers, backend):
    """One frame of every driver in `drivers` (all initialised and not finished; one library, and one handle each where they have
    estimator-state or FeatureManager slots): solve the current window, marginalise, slide, take in the next frame.  backend: how
    the solve, the residual query and the marginalisation are issued (OwnContexts, batch_stream.BatchedCalls).  Every slot call is
    made once for the group.  Returns, per driver, whether it has another frame."""
    est, fm = drivers[0].est, drivers[0].fm
    for d in drivers:
        if d.bias_relinearize is not None:
            d.repropagated.append(d.relinearize_biases())
    if est is not None:             # (state=dict(relinearize=): one relinearize_batch in front of the window call)
        est_relinearize(drivers)
        for d, win in zip(drivers, est.window_batch([d.est_slot for d in drivers])):
            d.pull_window(win)
    # [f_manager.triangulate,] vector2double, Solve(10)
    loaded = fm_windows(drivers, True) if fm is not None else [d.dict_windows(True) for d in drivers]
    for d, (w, _) in zip(drivers, loaded):
        d.ctx.load(w)
    reps = backend.solve(drivers)
    solved = [d.ctx.get_window() for d in drivers]
    if est is not None:             # double2vector + failureDetection of every window in one call
        for d, r in zip(drivers, est.update_batch([(d.est_slot, s[0], s[1], d.ext, True) for d, s in zip(drivers, solved)])):
            d.apply_update(r)
    else:
        for d, (w, _), (poses, sb, _) in zip(drivers, loaded, solved):
            d.poses, d.sb = anchor_gauge(w.poses, poses, sb)
    invds = [d.ctx.get_landmarks() for d in drivers]
    if fm is not None:
        fm_set_depths(drivers, invds)
    else:
        for d, (_, ids), invd in zip(drivers, loaded, invds):
            d.dict_set_depths(ids, invd)
    # FeaturePerId::is_outlier / solve_flag = 2 from the solved states the contexts hold, on the windows they were loaded with
    bad = [(d, [ids[k] for k in np.nonzero(f & 7)[0]])
           for d, (_, ids), f in zip(drivers, loaded, backend.flags(drivers, [w for w, _ in loaded])) if f is not None]
    kinds = []
    for d, rep in zip(drivers, reps):
        if d.prior is not None:      # estimator.cpp:1040-1049: b/err prior come back updated, H/Jt stay
            b, e = d.ctx.get_prior()
            d.prior = dict(d.prior, b=b[:156].copy(), err=e.copy())
        d.trajectory.append((d.s.times[d.frames[WINDOW_SIZE]], d.poses[WINDOW_SIZE].copy()))
        d.reports.append(rep)
        second_new = d.frames[WINDOW_SIZE - 1]
        margin_old = not (d.nonkey_every and second_new % d.nonkey_every == d.nonkey_every - 1)
        kinds.append(MARG_OLD if margin_old else MARG_SECOND_NEW)
        d.flags.append(kinds[-1])
    # backendOptimization marginalises on the re-anchored states (estimator.cpp:1086-1102)
    again = fm_windows(drivers, False) if fm is not None else [d.dict_windows(False) for d in drivers]
    priors = backend.marginalize(drivers, [(kind, w2, d.prior) for d, kind, (w2, _) in zip(drivers, kinds, again)])
    if bad:                         # removeOutlier + removeFailures, before the slides
        for d, ids in bad:
            d.record_rejected(ids)
        if fm is not None:
            fm_remove([d for d, _ in bad], [ids for _, ids in bad])
        else:
            for d, ids in bad:
                d.dict_remove(ids)
    more = []
    for d, p in zip(drivers, priors):
        d.prior = p
        more.append(d.next_frame < d.s.n_frames)
    go = [(d, kind == MARG_OLD) for d, m, kind in zip(drivers, more, kinds) if m]
    if not go:
        return more
    # slideWindow, then processIMU and the image of the next frame
    ds = [d for d, _ in go]
    if est is not None:
        slid = est.slide_batch([(d.est_slot, MARG_OLD if old else MARG_SECOND_NEW, True) for d, old in go])
        for d, r in zip(ds, slid):
            if not r["slid"]:
                raise RuntimeError("StreamDriver: the slot's window is not full (frame_count %d)" % r["frame_count"])
        mats = [(r["marg_R"], r["marg_P"], r["new_R"], r["new_P"]) if old else None for (_, old), r in zip(go, slid)]
    else:
        mats = [d.slide_mats() if old else None for d, old in go]
    if fm is not None:              # (both slide kinds ride in one slide_batch)
        fm_slide(ds, [FM_BACK_SHIFT_DEPTH if old else FM_FRONT for _, old in go], mats)
    else:
        for (d, old), m in zip(go, mats):
            if old:
                d.dict_slide_back_shift(m)
            else:
                d.dict_slide_front()
    for d, old in go:
        d.slide_lists(old)
    if est is not None:
        begun = [d.begin_next_frame() for d in ds]
        est.imu_batch([b[1] for b in begun])
        est.image_batch([b[2] for b in begun])
        new = [b[0] for b in begun]
    else:
        new = [d.propagate_next_frame() for d in ds]
    if fm is not None:
        fm_add(ds, new)
    else:
        for d, f in zip(ds, new):
            d.dict_add(f)
    return more


def init_round(group):
    """One INITIAL try of every driver in `group` (all created with `initialize`, not initialised yet, and alike in what one
    alignment call shares: batch_stream._init_group_key), every call made once for the group: the slots' queued feeding (est_flush),
    sfm_f (one tracks_batch), the alignment, each driver's own bookkeeping (init_apply), then visualInitialAlign's depth hand-over
    for the successes, the INITIAL slide, the next frame and its all_image_frame push for the failures, and the state hand-over
    (est_init_apply) for the successes."""
    lead = group[0]
    est, fm = lead.est, lead.fm
    if est is not None:             # the window in the first round, the last round's failures afterwards
        est_flush(group)
    tracks = fm_tracks(group) if fm is not None and lead.initialize.get("sfm") else [None] * len(group)
    reqs = [d.init_request(tr) for d, tr in zip(group, tracks)]
    res = lead.init_align([r[0] for r in reqs], [r[1] for r in reqs])
    won, lost = [], []
    for d, (item, _), r in zip(group, reqs, res):
        gone = d.init_apply(r)
        if gone is None:
            won.append((d, item, r))
        else:
            lost.append((d, gone))
    if won and fm is not None:
        fm_init_depths([d for d, _, _ in won], [item for _, item, _ in won], [float(r["s"]) for _, _, r in won])
    elif won:
        for d, item, r in won:
            d.dict_init_depths(item, float(r["s"]))
    if lost:                        # slideWindow in the INITIAL state: no prior, no depth shift (f_manager.removeBack); the next frame
        ds = [d for d, _ in lost]
        if fm is not None:
            fm_slide(ds, [FM_BACK] * len(ds))
            fm_add(ds, [d.frames[-1] for d in ds])
        else:
            for d, gone in lost:
                d.dict_slide_back(gone)
                d.dict_add(d.frames[-1])
        aif = [(d, gone) for d, gone in lost if d.aif is not None]
        rows = fm_tracks([d for d, _ in aif]) if aif and fm is not None else [None] * len(aif)
        for (d, gone), tr in zip(aif, rows):
            d._aif_push(len(d.frames) - 1, slide=d.s.times[gone], tracks=tr)
    if won and est is not None:
        est_init_apply([d for d, _, _ in won], [r for _, _, r in won])


class StreamDriver:
    def __init__(self, lib, stream, ctx_kwargs=None, pos_noise=0.02, rot_noise=0.005, depth_noise=0.05, seed=1,
                 triangulate=False, nonkey_every=0, outlier_px=None, bias_relinearize=None, initialize=None, state=None, features=None):
        """triangulate=True: a landmark's first depth comes from FeatureManager::triangulate (vio_triangulate, on the
        current pose estimates, feature_manager.cpp:203-257) the first time it enters a solve, as in
        Estimator::solveOdometry (estimator.cpp:489-503), instead of from the perturbed ground truth.
        nonkey_every=n > 0: every n-th frame is not a keyframe: when it is the second-newest frame of the window it is
        marginalised (MARGIN_SECOND_NEW) instead of the oldest one.
        outlier_px=x (HIP library only): after every solve the residual query (include/vio_residuals.h) flags the landmarks whose
        mean reprojection error exceeds x pixels, that have a point behind a camera, or whose inverse depth is not positive and finite;
        their tracks are erased after the marginalisation and before the slide — what removeOutlier (feature_manager.cpp:259-275) and
        removeFailures (:161-171) would do if they were active.  self.rejected: the count of every step.  None: no query.
        bias_relinearize=(ba_thresh, bg_thresh) (needs the GPU): the pre-integrations follow the bias estimates through the IMU
        library (include/vio_imu.h).  Every new interval, the merged one of a non-keyframe slide included, is pre-integrated at the bias
        of the frame it starts from (new IntegrationBase{acc_0, gyr_0, Bas[..], Bgs[..]}, estimator.cpp:116, 159, 1178, 1229), and
        before every solve the intervals whose start frame's bias moved more than the threshold (max-abs, per axis) from their
        linearized_ba / linearized_bg are re-propagated (repropagate, integration_base.h:38-52).  self.repropagated: the count of every
        step.  None: every interval stays at zero bias and the library is not loaded.
        initialize=dict(scale=, rot_noise=, pos_noise=, max_tries=, seed=) (needs the GPU): the window starts in the INITIAL state
        with no ground-truth state.  Each try aligns the current 11-frame window (every frame a keyframe) through the alignment
        library (include/vio_init.h) on visual_trajectory's SfM stand-in: gyro bias, re-propagation, LinearAlignment,
        RefineGravity (visualInitialAlign, estimator.cpp:384-460).  On success the state change is applied, the window's
        pre-integrations become the re-propagated ones, and the depths are triangulated on the un-scaled SfM poses with tic = 0 and
        then multiplied by s.  On failure the oldest frame leaves without a prior (the INITIAL slideWindow) and the next frame comes
        in; max_tries failures raise.  self.init_tries, self.init_frame (the newest frame at success) and self.init_result record it.
        An `aligner` entry (a callable(items, intervals, tic, g_norm, noise) returning the dicts InitHandle.initialize_batch returns)
        replaces the library (the CPU tests pass the numpy restatement).  An `sfm` entry makes the camera poses come from the
        window's feature tracks instead of visual_trajectory (scale, rot_noise, pos_noise and seed are then unused): True runs
        relativePose + GlobalSFM::construct through the SfM library (include/vio_sfm.h), a callable(items) returning the dicts
        SfmHandle.sfm_batch returns replaces it; a window whose SfM fails counts as a failed try with status sfm.TRY_FAILED_SFM + |SfM status| and the
        SfM status under `sfm_status` (self.init_sfm_status records every try's SfM status).  A `calibrate_ric` entry (with `sfm`)
        starts from an unknown camera-IMU rotation: self.ext[3:7] is the identity and the stream's own rotation is not used.  Each
        try first calibrates it on the window's tracks and the delta_q of its pre-integrations (include/vio_exrot.h,
        InitialEXRotation::CalibrationExRotation); on success self.ext[3:7] is set before the SfM and the alignment, on failure the try
        counts as failed with status exrot.TRY_FAILED_EXROT + |status| and the calibration's status under `exrot_status`
        (self.init_exrot_status records every try's).  True: the library's defaults; a dict(min_sigma=, min_frames=, huber_deg=):
        its gate; a callable(items) returning the dicts ExrotHandle.exrot_batch returns replaces the library.  An `all_frames` entry
        (with `sfm`), (aif_handle, slot): the window's images and samples are fed into slot `slot` of an aif.AifHandle
        (include/vio_aif.h) while the driver is in the INITIAL state, and every try comes from aif.initialize_from_frames over that
        slot (the structure call on the SfM's result, the gyro bias, the re-propagation and the alignment) instead of
        InitHandle.initialize_batch over the driver's lists; a key walk or PnP that fails is a failed try with status
        sfm.TRY_FAILED_SFM.  The slot is fed in steps that are queued and sent in front of a try, for every driver of a group in
        one call each (aif_flush).  The handle's IMU noise is the caller's to set (AifHandle.set_config) and must equal the
        stream's; an `aligner` cannot be combined with `all_frames` (both raise ValueError).  A `state` entry, (est_handle, slot) or
        the dict form of state= below: the stream lives in slot `slot` of an est.EstHandle from its first IMU sample.  The slot is reset
        and fed as processIMU / processImage would feed it (one sample in front of the first image for acc_0 / gyr_0, then each window
        frame's samples and its header), in queued steps that est_flush sends for every driver of a group in one call each; a failed try
        queues slideWindow (MARG_OLD), the next frame's samples and its header; a successful one ends in init_apply_batch
        (include/vio_est_init.h, with commit_last) on the try's poses, speed_bias, g and rot, and from then on the driver is a state=
        driver: the first update_batch commits last_R / last_P / last_R0 / last_P0 again (estimator.cpp:234-237).  It composes with `all_frames` and
        features=.  None: the ground-truth start below.
        state=(est_handle, slot): the window states, the intervals' samples and pre-integrations live in slot `slot` of an
        est.EstHandle (include/vio_est.h; or anything with its batched methods): the ground-truth start is written there as an
        initialisation result would be, every step reads the window from it (vector2double and the ten records), re-anchors through it
        (double2vector, with failureDetection's verdict appended to self.failures; a failure raises, there is no reboot policy here),
        slides through it and feeds the next interval's samples to its processIMU.  Not with initialize= or bias_relinearize=.
        state=dict(handle=, slot=, relinearize=(ba_thresh, bg_thresh)): the same, and with `relinearize` the slot's pre-integrations follow
        the bias estimates as bias_relinearize= makes the driver's own do: one relinearize_batch (include/vio_est_init.h) in front of every
        window pull; self.repropagated: the count of every step.  No IMU-library handle is created.  (After a non-keyframe slide the slot's
        merged interval keeps its linearisation biases, as the reference's push_back does, where bias_relinearize= re-integrates it at
        the frame's bias.)
        features=(fm_handle, slot), or dict(handle=, slot=, remove_failures=False): the FeatureManager lives in slot `slot` of an
        fm.FmHandle (include/vio_fm.h and vio_fm_stream.h; or anything with its batched methods) and the driver holds no tracks /
        depth dicts.  The slot is reset and fed every stream observation of the eleven window frames (add_batch, frame_count 0 .. 10;
        ids are landmark numbers); a step exports the window arrays with triangulation (export_batch), writes the solved inverse
        depths back (set_depth_batch; remove_failures=True also erases the tracks solved to a negative depth, as the reference's
        removeFailures does), exports the marginalisation's edges, slides (slide_batch: BACK_SHIFT_DEPTH on the four arrays of
        slideWindowOld, FRONT for a non-keyframe) and adds the next frame.  An INITIAL try reads sfm_f with tracks_batch, a failed
        one slides with BACK, a successful one ends in init_depth_batch on the SfM poses with tic = 0 and s.  The library's own
        keyframe decision of every add is recorded in self.fm_keyframe and not used.  A slot status other than OK raises.  With
        outlier_px the flagged landmarks' feature ids (the export's) go to remove_batch (include/vio_fm_outlier.h) after the
        marginalisation and before the slide; self.fm_erased: the rows each call erased (an id that remove_failures=True had erased
        already counts in self.rejected and not here).  A handle without remove_batch raises ValueError with outlier_px.  Not with
        triangulate=False unless initialize= is given (ValueError): the perturbed ground-truth depths are not FeatureManager
        behaviour."""
        if state is not None and (initialize is not None or bias_relinearize is not None):
            raise ValueError("StreamDriver: state= cannot be combined with initialize= or bias_relinearize=")
        self.fm, self.fm_slot, self.fm_remove_failures = None, None, False
        if features is not None:
            if not triangulate and initialize is None:
                raise ValueError("StreamDriver: features= needs triangulate=True or initialize= (the perturbed ground-truth depths are not a FeatureManager behaviour)")
            if isinstance(features, dict):
                self.fm, self.fm_slot = features["handle"], int(features["slot"])
                self.fm_remove_failures = bool(features.get("remove_failures", False))
            else:
                self.fm, self.fm_slot = features[0], int(features[1])
            if outlier_px is not None and not hasattr(self.fm, "remove_batch"):
                raise ValueError("StreamDriver: features= with outlier_px needs a handle with remove_batch (removeOutlier by id, include/vio_fm_outlier.h)")
        self._rejected = set()      # landmarks whose tracks were erased (outlier_px set): frame_points leaves them out
        self.fm_keyframe = []       # addFeatureCheckParallax's own decision of every frame added (features set): recorded, not used
        self.lib, self.s = lib, stream
        self.noise = dict(getattr(stream, "noise", None) or {})      # sensor noise of re-integrated intervals (default: synth's)
        self.g_norm = float(getattr(stream, "g_norm", synth.G_NORM))
        kw = dict(ctx_kwargs or {})
        if hasattr(stream, "g_norm"):
            kw.setdefault("gravity", (0.0, 0.0, self.g_norm))
        self.ctx = lib.context(**kw)
        rng = np.random.RandomState(seed)
        st = stream
        self.frames = list(range(NUM_FRAMES))              # global index of the frame in each window slot
        self.intervals = [dict(st.imu[k]) for k in range(WINDOW_SIZE)]     # raw IMU between consecutive window frames
        self.preint = [st.preint[k] for k in range(WINDOW_SIZE)]
        self.next_frame = NUM_FRAMES
        self.nonkey_every = nonkey_every
        self.poses = np.zeros((NUM_FRAMES, 7))
        self.sb = np.zeros((NUM_FRAMES, 9))
        for i in range(NUM_FRAMES if initialize is None else 0):
            th = rng.normal(0.0, rot_noise, 3)
            dq = np.array([th[0] / 2, th[1] / 2, th[2] / 2, 1.0])
            dq /= np.linalg.norm(dq)
            self.poses[i, 0:3] = st.P[i] + rng.normal(0.0, pos_noise, 3)
            self.poses[i, 3:7] = synth.quat_mul(st.Q[i], dq)
            self.sb[i, 0:3] = st.V[i]
        self.ext = st.ext.copy()
        if initialize is not None and initialize.get("calibrate_ric"):
            if not initialize.get("sfm"):
                raise ValueError("StreamDriver: calibrate_ric needs sfm (the stand-in's poses are made with the true rotation)")
            self.ext[3:7] = (0.0, 0.0, 0.0, 1.0)
        # tracks (FeaturePerId): landmark -> list of (global frame, normalised point), the first one is the host
        if self.fm is not None:                            # (the slot holds them)
            self.fm.reset(self.fm_slot)
            for k, f in enumerate(self.frames):
                fm_add([self], [f], k)
        else:
            self.tracks = {}
            for f in self.frames:
                self.dict_add(f)
            self.depth = {}                                # landmark -> estimated depth in its current host frame
        self.init_depth = np.array(st.lm_depth) * (1.0 + depth_noise * st.init_noise)
        self.triangulate = triangulate
        self.prior = None
        self.trajectory = []        # (stamp, pose[7]) of the newest frame after every solve
        self.reports = []
        self.flags = []             # marginalisation flag of every step
        self.n_triangulated = 0
        self.outlier_px = outlier_px
        self.rejected = []          # tracks erased at every step (outlier_px set)
        self.rejected_ids = []      # ... and which
        self.fm_erased = []         # rows every remove_batch erased (features and outlier_px set)
        self.bias_relinearize = None if bias_relinearize is None else (float(bias_relinearize[0]), float(bias_relinearize[1]))
        self.repropagated = []      # intervals re-propagated before every solve (bias_relinearize set)
        if self.bias_relinearize is not None:
            from . import load_imu
            self.imu_h = load_imu().create(device=self.ctx.cfg.device)
            self._imu_stale = True              # the handle does not hold self.intervals
            self._repropagate(list(range(WINDOW_SIZE)))
        self.initialize = None if initialize is None else dict(initialize)
        self.initialized = initialize is None
        self.init_tries, self.init_frame, self.init_result = 0, None, None
        if self.initialize is not None:
            cfg = dict(scale=1.0, rot_noise=0.0, pos_noise=0.0, max_tries=10, seed=0)
            cfg.update(self.initialize)
            self.initialize = cfg
            self._init_h = self._init_imu = self._sfm_h = self._exrot_h = None
            self.init_sfm_status = []
            self.init_exrot_status = []
        self.aif, self.aif_slot = None, None
        if self.initialize is not None and self.initialize.get("all_frames") is not None:
            if not self.initialize.get("sfm"):
                raise ValueError("StreamDriver: all_frames needs sfm (initialStructure's frame work starts from the SfM)")
            if self.initialize.get("aligner") is not None:
                raise ValueError("StreamDriver: all_frames takes the try from the library (aif.initialize_from_frames); it cannot be combined with an aligner")
            self.aif, self.aif_slot = self.initialize["all_frames"][0], int(self.initialize["all_frames"][1])
            nz = self._noise()
            held = getattr(self.aif, "noise", None)         # (an AifHandle remembers its set_config; a stand-in without one is not checked)
            if held is not None and tuple(float(nz[k]) for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")) != tuple(float(v) for v in held):
                raise ValueError("StreamDriver: the stream's IMU noise differs from the all_frames handle's (AifHandle.set_config); the slot's records would not be the driver's")
            self._aif_seed()
        init_state = None if self.initialize is None else self.initialize.get("state")
        self.est, self.est_slot, self.est_relin = (None, None, None) if state is None and init_state is None else _parse_state(state if state is not None else init_state)
        self.failures = []          # failureDetection's verdict of every step (state set): the update's result dicts
        if init_state is not None:  # the slot in the INITIAL state: fed by est_flush, handed over by est_init_apply
            self._est_seed_initial()
        elif self.est is not None:
            self._seed_state()

    # ---- the window state in an estimator-state slot (state) -------------------------------------------
    def _seed_state(self):
        """The ground-truth start as a full window in the slot: frame_count = WINDOW_SIZE, interval j + 1 = self.intervals[j] at zero
        linearisation biases, last_R / last_P / last_R0 / last_P0 as after a first solve (estimator.cpp:198-201)."""
        self._est_config()
        g = (0.0, 0.0, self.g_norm)
        ivs = self.intervals
        off = np.concatenate([[0, 0], np.cumsum([len(iv["dt"]) for iv in ivs])]).astype(np.int64)
        S = int(off[-1])
        cat = lambda key, w: np.concatenate([np.asarray(iv[key], dtype=np.float64).reshape(-1, w) for iv in ivs]).reshape(S, w)
        R = np.array([synth.quat_to_rot(q).reshape(9) for q in self.poses[:, 3:7]])
        first = np.zeros((NUM_FRAMES, 6))
        for j, iv in enumerate(ivs):
            first[j + 1, 0:3], first[j + 1, 3:6] = iv["acc0"], iv["gyr0"]
        acc, gyr = cat("acc", 3), cat("gyr", 3)
        self.est.state_set(self.est_slot, dict(
            frame_count=WINDOW_SIZE, first_imu=1, failure_occur=0, exists=np.ones(NUM_FRAMES, dtype=np.int32), Ps=self.poses[:, 0:3], Rs=R,
            Vs=self.sb[:, 0:3], Bas=self.sb[:, 3:6], Bgs=self.sb[:, 6:9], Headers=np.array([self.s.times[f] for f in self.frames], dtype=np.float64),
            tic=self.ext[0:3], ric=synth.quat_to_rot(self.ext[3:7]).reshape(9), g=np.array(g), acc_0=acc[-1], gyr_0=gyr[-1], first=first,
            lin_bias=np.zeros((NUM_FRAMES, 6)), last_R=R[WINDOW_SIZE], last_P=self.poses[WINDOW_SIZE, 0:3], last_R0=R[0],
            last_P0=self.poses[0, 0:3], off=off, dt=cat("dt", 1).reshape(S), acc=acc, gyr=gyr))

    def _noise(self):
        """The four IMU noise figures a slot's handle is configured with: synth's, overridden by the stream's."""
        nz = dict(acc_n=synth.ACC_N, gyr_n=synth.GYR_N, acc_w=synth.ACC_W, gyr_w=synth.GYR_W)
        nz.update(self.noise)
        return nz

    def _est_config(self):
        self.est.set_config(self.ext[0:3], self.ext[3:7], (0.0, 0.0, self.g_norm), self._noise())

    @staticmethod
    def _est_samples(iv):
        return (np.array(iv["dt"], dtype=np.float64), np.array(iv["acc"], dtype=np.float64).reshape(-1, 3), np.array(iv["gyr"], dtype=np.float64).reshape(-1, 3))

    def _est_seed_initial(self):
        """The slot reset, and the window as the INITIAL state has seen it queued for it (slide, imu, image per step): one sample in
        front of the first image, which gives acc_0 / gyr_0 and constructs interval 0; then every window frame's samples and header."""
        self._est_config()
        self.est.reset(self.est_slot)
        iv0 = self.intervals[0]
        self._est_queue = [(None, (np.zeros(1), np.array(iv0["acc0"], dtype=np.float64).reshape(1, 3), np.array(iv0["gyr0"], dtype=np.float64).reshape(1, 3)),
                            (float(self.s.times[self.frames[0]]), True))]
        for k in range(1, len(self.frames)):
            self._est_queue.append((None, self._est_samples(self.intervals[k - 1]), (float(self.s.times[self.frames[k]]), True)))

    def pull_window(self, win=None):
        """poses, speed-biases and the ten pre-integrations from the slot (win: this slot's entry of a batched window call)."""
        if win is None:
            win = self.est.window_batch([self.est_slot])[0]
        self.poses, self.sb = np.array(win["poses"], dtype=np.float64), np.array(win["speed_bias"], dtype=np.float64)
        self.preint = [p if isinstance(p, dict) else record_dict(p) for p in win["preint"]]

    def apply_update(self, res):
        """What double2vector + failureDetection returned for this slot: the re-anchored window and the verdict."""
        self.failures.append({k: res[k] for k in ("failure", "gate", "singular")})
        self.poses, self.sb = np.array(res["poses"], dtype=np.float64), np.array(res["speed_bias"], dtype=np.float64)
        if res["failure"]:
            raise RuntimeError("StreamDriver: failureDetection fired (gate %d) at frame %d; no reboot policy here" % (res["gate"], self.frames[-1]))

    def begin_next_frame(self):
        """The next frame's number and the processIMU / processImage items that bring it into the slot."""
        f = self.next_frame
        self.next_frame += 1
        iv = self.s.imu[self.frames[-1]]
        self.frames.append(f)
        return f, (self.est_slot, iv["dt"], iv["acc"], iv["gyr"]), (self.est_slot, float(self.s.times[f]), False)

    # ---- initialisation (initialize) ------------------------------------------------------------------
    def _aif_push(self, k, slide=None, first=None, tracks=None):
        """Queues window frame k for the all_image_frame slot as one step (slide, imu, image): the erase up to header `slide`
        (slideWindow) if given, the samples since frame k - 1 (processIMU; `first`: one sample in front of the first image), then the
        image (processImage).  tracks (features set): this slot's entry of a tracks call; None: the driver's own dicts.  aif_flush
        feeds the queued steps of many drivers in one call each."""
        f = self.frames[k]
        iv = first if k == 0 else self.intervals[k - 1]
        imu = None if iv is None else (np.array(iv["dt"], dtype=np.float64), np.array(iv["acc"], dtype=np.float64), np.array(iv["gyr"], dtype=np.float64))
        # a track's observations are consecutive window frames from its first one, so frame k's is entry k - (index of that first frame):
        # one look per track, not a scan of its list
        if tracks is not None:      # the slot's rows that have window frame k
            has = (tracks["start"] <= k) & (k < tracks["start"] + np.diff(tracks["off"]))
            ids = np.array(tracks["ids"][has], dtype=np.int64)
            pts = np.array(tracks["pts"][(tracks["off"][:-1] + k - tracks["start"])[has]], dtype=np.float64).reshape(-1, 2)
        else:
            pos = {fr: i for i, fr in enumerate(self.frames)}
            obs = []
            for l, tr in self.tracks.items():
                j = k - pos[tr[0][0]]
                if 0 <= j < len(tr):
                    if tr[j][0] != f:
                        raise RuntimeError("StreamDriver: track %d is not consecutive in the window's frames" % l)
                    obs.append((l, tr[j][1]))
            ids = np.array([l for l, _ in obs], dtype=np.int64)
            pts = np.array([p for _, p in obs], dtype=np.float64).reshape(-1, 2)
        image = (float(self.s.times[f]), ids, pts, self.sb[k, 3:6].copy(), self.sb[k, 6:9].copy())
        self._aif_queue.append((None if slide is None else (float(slide),), imu, image))

    def _aif_seed(self):
        """The window as the INITIAL state has seen it, queued for the slot.  One sample in front of the first image carries the first
        interval's acc_0 / gyr_0 (it is dropped: no image yet; acc_0 / gyr_0 follow)."""
        self.aif.reset(self.aif_slot)
        self._aif_queue = []
        iv = self.intervals[0]
        tr = fm_tracks([self])[0] if self.fm is not None else None
        for k in range(len(self.frames)):
            self._aif_push(k, first=dict(dt=[0.0], acc=[iv["acc0"]], gyr=[iv["gyr0"]]), tracks=tr)

    def init_request(self, tracks=None):
        """The current window as an alignment item (visual_trajectory's R / T, the zero-bias records) and its raw intervals.  tracks
        (features set): this slot's entry of a batched tracks call."""
        c = self.initialize
        if c.get("sfm"):            # R / T are filled in by init_align's SfM call
            from .sfm import item_from_tracks
            if self.fm is not None:     # sfm_f is the slot's list as it stands
                tr = fm_tracks([self])[0] if tracks is None else tracks
                sfm_item = dict(n_frames=len(self.frames), start_frame=np.array(tr["start"], dtype=np.int32),
                                obs_offset=np.array(tr["off"], dtype=np.int64), pts=np.array(tr["pts"], dtype=np.float64).reshape(-1, 2))
                item = dict(sfm_item=sfm_item, owner=self, R=None, T=None, pre=list(self.preint), is_key=None,
                            fm_ids=np.array(tr["ids"], dtype=np.int64))
            else:
                item = dict(sfm_item=item_from_tracks(self.tracks, self.frames)[0], owner=self, R=None, T=None, pre=list(self.preint),
                            is_key=None)
            if c.get("calibrate_ric"):
                from .exrot import delta_q_wxyz
                item["exrot_item"] = dict(item["sfm_item"], delta_q=delta_q_wxyz(self.preint))
            return item, list(self.intervals)
        R, T = visual_trajectory(self.s, self.frames, 0, c["scale"], c["rot_noise"], c["pos_noise"], c["seed"] + self.init_tries)
        return dict(R=R, T=T, pre=list(self.preint), is_key=None), list(self.intervals)

    def init_sfm(self, items):
        """One SfM call for every item made with `sfm`: fills in R = Q RIC^T and T (estimator.cpp:316-318) where it succeeds.
        Returns each item's SfM status."""
        from .sfm import sfm_items_to_init_items
        c = self.initialize
        if callable(c["sfm"]):
            res = c["sfm"]([it["sfm_item"] for it in items])
        else:
            if self._sfm_h is None:
                from . import load_sfm
                self._sfm_h = load_sfm().create(device=self.ctx.cfg.device)
            res = self._sfm_h.sfm_batch([it["sfm_item"] for it in items])
        for it, r in zip(items, res):
            it["sfm_result"] = r
            ric = synth.quat_to_rot(it["owner"].ext[3:7])
            done = sfm_items_to_init_items([r], ric, [it["pre"]])[0]
            if done is not None:
                it["R"], it["T"] = done["R"], done["T"]
        return [int(r["status"]) for r in res]

    def init_exrot(self, items):
        """One calibration call for every item made with `calibrate_ric`: sets the owner's ext[3:7] where it succeeds.  Returns each
        item's calibration status."""
        c = self.initialize
        cal = c["calibrate_ric"]
        if callable(cal):
            res = cal([it["exrot_item"] for it in items])
        else:
            if self._exrot_h is None:
                from . import load_exrot
                self._exrot_h = load_exrot().create(device=self.ctx.cfg.device)
                if isinstance(cal, dict):
                    self._exrot_h.set_config(**cal)
            res = self._exrot_h.exrot_batch([it["exrot_item"] for it in items])
        for it, r in zip(items, res):
            if r["status"] == 0:
                w, x, y, z = r["q"]
                it["owner"].ext[3:7] = (x, y, z, w)
                it["owner"].init_exrot_result = r
        return [int(r["status"]) for r in res]

    def init_align(self, items, intervals):
        """The alignment of `items` on this driver's backend: the library (one handle pair per driver), or the `aligner` given."""
        c = self.initialize
        if c.get("sfm"):
            from .sfm import TRY_FAILED_SFM
            out = [None] * len(items)
            live = list(range(len(items)))
            if c.get("calibrate_ric"):
                from .exrot import TRY_FAILED_EXROT
                xs = self.init_exrot(items)
                for i, st in enumerate(xs):
                    items[i]["owner"].init_exrot_status.append(st)
                    if st != 0:
                        out[i] = dict(status=TRY_FAILED_EXROT + abs(st), exrot_status=st)     # a calibration failure: a failed try
                live = [i for i in live if xs[i] == 0]
            sts = self.init_sfm([items[i] for i in live]) if live else []
            ok = []
            for i, st in zip(live, sts):
                items[i]["owner"].init_sfm_status.append(st)
                out[i] = dict(status=TRY_FAILED_SFM + abs(st), sfm_status=st)               # an SfM failure: a failed try
                if st == 0:
                    ok.append(i)
            if ok and c.get("all_frames") is not None:
                for i, r in zip(ok, self._init_from_frames([items[i] for i in ok])):
                    out[i] = r
            elif ok:
                plain = [{k: v for k, v in items[i].items() if k not in ("sfm_item", "exrot_item", "owner", "sfm_result", "fm_ids")} for i in ok]
                for i, r in zip(ok, self._init_align(plain, [intervals[i] for i in ok])):
                    out[i] = r
            return out
        return self._init_align(items, intervals)

    def _init_from_frames(self, items):
        """One try of every item's owner from its all_image_frame slot (aif.initialize_from_frames: four calls for the group).  The
        items' R / T become the structure call's; a slot whose key walk or PnP failed is a failed try."""
        from .aif import BatchImageFrames, initialize_from_frames
        from .sfm import TRY_FAILED_SFM, item_from_tracks
        if self._init_h is None:
            from . import load_init
            self._init_h = load_init().create(device=self.ctx.cfg.device)
        owners = [it["owner"] for it in items]
        aif_flush(owners)
        res = initialize_from_frames(BatchImageFrames(self.aif, [d.aif_slot for d in owners]), self._init_h, [it["sfm_result"] for it in items],
                                     [[float(d.s.times[f]) for f in d.frames] for d in owners],
                                     [it["fm_ids"] if d.fm is not None else np.array(item_from_tracks(d.tracks, d.frames)[1], dtype=np.int64)
                                      for d, it in zip(owners, items)],
                                     np.stack([synth.quat_to_rot(d.ext[3:7]) for d in owners]), self.ext[0:3].copy(), self.g_norm)
        out = []
        for it, r in zip(items, res):
            if r is None:
                out.append(dict(status=TRY_FAILED_SFM, sfm_status=0))
                continue
            it["R"], it["T"] = r["structure"]["R"], r["structure"]["T"]
            out.append(r)
        return out

    def _init_align(self, items, intervals):
        c = self.initialize
        if c.get("aligner") is not None:
            return c["aligner"](items, intervals, self.ext[0:3].copy(), self.g_norm, self.noise)
        if self._init_h is None:
            from . import load_imu, load_init
            self._init_h = load_init().create(device=self.ctx.cfg.device)
            self._init_imu = load_imu().create(device=self.ctx.cfg.device)
        return self._init_h.initialize_batch(items, intervals, self._init_imu, self.ext[0:3].copy(), self.g_norm, self.noise)

    def init_apply(self, res):
        """The driver's own bookkeeping of one try's outcome, none of it on a handle (init_round makes the slots' calls and the
        FeatureManager's part).  Success: visualInitialAlign's state change; returns None.  Failure: the INITIAL slideWindow of the
        window lists (the oldest frame leaves, no prior), the next frame's propagation and, with initialize=dict(state=), the queue
        entry that brings both into the slot; returns the global frame that left the window."""
        self.init_tries += 1
        if res["status"] == 0:
            self.poses = np.asarray(res["poses"], dtype=np.float64).reshape(NUM_FRAMES, 7).copy()
            self.sb = np.asarray(res["speed_bias"], dtype=np.float64).reshape(NUM_FRAMES, 9).copy()
            self.preint = list(res["pre"])
            self.init_result = res
            self.init_frame = self.frames[WINDOW_SIZE]
            self.initialized = True
            return None
        if self.init_tries >= self.initialize["max_tries"]:
            raise RuntimeError("StreamDriver: no initialisation after %d tries (last status %d)" % (self.init_tries, res["status"]))
        if self.next_frame >= self.s.n_frames:
            raise RuntimeError("StreamDriver: the stream ended before the initialisation succeeded")
        gone = self.frames[0]
        self._drop_oldest()
        self.propagate_next_frame()
        if self.est is not None:    # slideWindow, processIMU over the new interval, processImage: frame_count stays WINDOW_SIZE
            self._est_queue.append(((MARG_OLD, False), self._est_samples(self.intervals[-1]), (float(self.s.times[self.frames[-1]]), True)))
        return gone

    def ensure_initialized(self):
        """Tries until the window is initialised (a no-op for a driver created without `initialize`, or already initialised): rounds
        of a group of one.  With initialize=dict(state=) the queued feeding of the slot goes out at the head of every round, so a
        driver that raises after max_tries has fed its slot."""
        while not self.initialized:
            init_round([self])

    # ---- feature bookkeeping (FeatureManager) ---------------------------------------------------------
    def frame_points(self, f):
        """Every stream observation of global frame f as the front end would hand it over: (ids, points), ids the landmark numbers,
        the point lm_px for the frame that hosts the landmark, else lm_obs[l][f].  A landmark whose track was rejected (outlier_px)
        is left out from then on, as dict_add leaves it out of the dicts: an erased track is not begun again."""
        st = self.s
        ids, pts = [], []
        for l, h in enumerate(st.lm_host):
            if l in self._rejected:
                continue
            if h == f:
                ids.append(l); pts.append(st.lm_px[l])
            elif f in st.lm_obs[l]:
                ids.append(l); pts.append(st.lm_obs[l][f])
        return np.array(ids, dtype=np.int64), np.array(pts, dtype=np.float64).reshape(-1, 2)

    # The FeatureManager a driver without features= keeps in its own tracks / depth dicts: one method per operation, beside the fm_*
    # helpers that make the same operation in the slots of a group (step_group and init_round choose once per operation).
    def dict_add(self, f):
        """fm_add: global frame f's observations begin or extend their tracks."""
        st = self.s
        for l, h in enumerate(st.lm_host):
            if h == f:
                self.tracks[l] = [(f, np.asarray(st.lm_px[l], dtype=np.float64))]
            elif l in self.tracks and f in st.lm_obs[l] and self.tracks[l][-1][0] == self.prev_of(f):
                self.tracks[l].append((f, np.asarray(st.lm_obs[l][f], dtype=np.float64)))

    def dict_windows(self, triangulate):
        """fm_windows: (Window, feature ids) on the current poses, the tracks without a depth given one first (triangulate)."""
        if triangulate:
            self.ensure_depths()
        return self.window_arrays()

    def dict_set_depths(self, ids, inv_depths):
        """fm_set_depths: setDepth from the solved inverse depths of landmarks `ids`."""
        for l, v in zip(ids, inv_depths):
            self.depth[l] = 1.0 / v

    def dict_remove(self, ids):
        """fm_remove: removeOutlier / removeFailures by landmark."""
        for l in ids:
            del self.tracks[l]
            self.depth.pop(l, None)

    def dict_slide_back(self, gone):
        """fm_slide(FM_BACK): removeBack, global frame `gone` leaves the front of its tracks (the INITIAL slideWindow)."""
        for l in list(self.tracks.keys()):
            tr = self.tracks[l]
            if tr[0][0] == gone:
                del tr[0]
                if not tr:
                    del self.tracks[l]

    def dict_slide_back_shift(self, mats):
        """fm_slide(FM_BACK_SHIFT_DEPTH): removeBackShiftDepth (feature_manager.cpp:276-312) on slideWindowOld's four arrays, before
        the window lists slide.  (numpy's products: fm_shift_depth evaluates the shift in another order.)"""
        gone = self.frames[0]
        mR, mP, nR, nP = mats
        for l in list(self.tracks.keys()):
            tr = self.tracks[l]
            if tr[0][0] != gone:
                continue
            uv = np.array([tr[0][1][0], tr[0][1][1], 1.0])
            del tr[0]
            if len(tr) < 2:
                del self.tracks[l]
                self.depth.pop(l, None)
                continue
            if l in self.depth:
                pj = nR.T @ (mR @ (uv * self.depth[l]) + mP - nP)
                self.depth[l] = float(pj[2]) if pj[2] > 0 else 5.0       # INIT_DEPTH

    def dict_slide_front(self):
        """fm_slide(FM_FRONT): removeFront (feature_manager.cpp:331-350) of the second-newest frame, before the window lists slide."""
        gone = self.frames[WINDOW_SIZE - 1]
        for l in list(self.tracks.keys()):
            tr = [o for o in self.tracks[l] if o[0] != gone]
            if not tr:
                del self.tracks[l]
                self.depth.pop(l, None)
            else:
                self.tracks[l] = tr

    def dict_init_depths(self, item, s):
        """fm_init_depths: f_manager.clearDepth; triangulate on the SfM poses with TIC_TMP = 0 and RIC; estimated_depth *= s
        (estimator.cpp:407-439)."""
        self.depth = {}
        todo = self.usable()
        for (l, _), v in zip(todo, self._triangulate(todo, sfm_poses(item), np.concatenate([np.zeros(3), self.ext[3:7]]))):
            self.depth[l] = float(v) * s

    def _triangulate(self, todo, poses, ext):
        """The depths of tracks todo = [(landmark, window index of its host)] by the context's triangulation on `poses` and `ext`."""
        if not todo:
            return []
        sf, off, pts = [], [0], []
        for l, start in todo:
            sf.append(start); pts.extend(p for _, p in self.tracks[l]); off.append(off[-1] + len(self.tracks[l]))
        self.n_triangulated += len(todo)
        return self.ctx.triangulate(np.array(sf, dtype=np.int32), np.array(off, dtype=np.int64), np.array(pts).reshape(-1, 2),
                                    poses, ext, -np.ones(len(todo)))

    def prev_of(self, f):
        """The window frame in front of global frame f (tracks are consecutive in window frames)."""
        fr = self.frames if f in self.frames else self.frames + [f]
        i = fr.index(f)
        return fr[i - 1] if i > 0 else None

    def usable(self):
        """(landmark, window index of its host) of the tracks the optimiser takes: used_num >= 2 and
        start_frame < WINDOW_SIZE - 2 (estimator.cpp:979-981)."""
        out = []
        for l, tr in self.tracks.items():
            start = self.frames.index(tr[0][0])
            if len(tr) >= 2 and start < WINDOW_SIZE - 2:
                out.append((l, start))
        return out

    def ensure_depths(self):
        """First depth of the tracks that have none: triangulation on the current poses, or perturbed ground truth."""
        todo = [(l, start) for l, start in self.usable() if l not in self.depth]
        if not todo:
            return
        if not self.triangulate:
            for l, _ in todo:
                self.depth[l] = float(self.init_depth[l])
            return
        for (l, _), v in zip(todo, self._triangulate(todo, self.poses, self.ext)):
            self.depth[l] = float(v)

    def window_arrays(self):
        ids, lm, host, target, pi, pj, invd = [], [], [], [], [], [], []
        for l, start in self.usable():
            k = len(ids)
            ids.append(l)
            invd.append(1.0 / self.depth[l])
            tr = self.tracks[l]
            for j in range(1, len(tr)):
                lm.append(k); host.append(start); target.append(start + j); pi.append(tr[0][1]); pj.append(tr[j][1])
        w = synth.Window(poses=self.poses.copy(), speed_bias=self.sb.copy(), ext=self.ext.copy(),
                         inv_depth=np.array(invd), lm=np.array(lm, dtype=np.int32),
                         host=np.array(host, dtype=np.int32), target=np.array(target, dtype=np.int32),
                         pts_i=np.array(pi).reshape(-1, 2), pts_j=np.array(pj).reshape(-1, 2),
                         preint=list(self.preint), prior=self.prior,
                         n_landmarks=len(ids), n_observations=len(lm))
        return w, ids

    @property
    def inv_depth(self):
        """Inverse depths by landmark id (NaN where the landmark never got one) — what the tests compare."""
        out = np.full(len(self.s.lm_host), np.nan)
        ids, depths = self._depths()
        out[ids] = 1.0 / depths
        return out

    @property
    def have_depth(self):
        out = np.zeros(len(self.s.lm_host), dtype=bool)
        out[self._depths()[0]] = True
        return out

    def _depths(self):
        """(landmark ids, depths) of the landmarks that have a depth: the dicts', or the slot's rows (-1 until a row gets one)."""
        if self.fm is None:
            return np.array(list(self.depth.keys()), dtype=np.int64), np.array(list(self.depth.values()), dtype=np.float64)
        tr = fm_tracks([self])[0]
        got = tr["depth"] != -1.0
        return tr["ids"][got], tr["depth"][got]

    # ---- IMU pre-integration at the bias estimates (bias_relinearize) ---------------------------------
    def _repropagate(self, ks):
        """Pre-integrate intervals ks of the window at the bias of the frame each starts from (interval k: frame k -> k + 1)."""
        if self._imu_stale:
            self.imu_h.load(self.intervals, self.noise)
            self._imu_stale = False
        n = len(self.intervals)
        recs = self.imu_h.propagate(self.sb[:n, 3:6], self.sb[:n, 6:9], which=ks)
        for k, r in zip(ks, recs):
            self.preint[k] = record_dict(r)

    def relinearize_biases(self):
        """repropagate the intervals whose start frame's bias moved past the thresholds; returns how many."""
        tba, tbg = self.bias_relinearize
        ks = [k for k in range(WINDOW_SIZE)
              if np.abs(self.sb[k, 3:6] - self.preint[k]["linearized_ba"]).max() > tba
              or np.abs(self.sb[k, 6:9] - self.preint[k]["linearized_bg"]).max() > tbg]
        if ks:
            self._repropagate(ks)
        return len(ks)

    # ---- one frame ------------------------------------------------------------------------------------
    def step(self):
        """Solve the current window, marginalise, slide, take in the next frame.  Returns False at the end."""
        self.ensure_initialized()
        return step_group([self], OwnContexts())[0]

    def record_rejected(self, bad):
        """The tracks the residual query's flags condemn at this step, counted and listed (their erasure is the FeatureManager's:
        fm_remove or dict_remove)."""
        self.rejected.append(len(bad))
        self.rejected_ids.extend(bad)
        self._rejected.update(bad)

    def slide_mats(self):
        """The four arrays of slideWindowOld (marg_R, marg_P, new_R, new_P) from the poses of the two oldest frames (a state= driver
        takes the slot's)."""
        R0 = synth.quat_to_rot(self.poses[0, 3:7]); R1 = synth.quat_to_rot(self.poses[1, 3:7])
        ric, tic = synth.quat_to_rot(self.ext[3:7]), self.ext[0:3]
        return R0 @ ric, self.poses[0, 0:3] + R0 @ tic, R1 @ ric, self.poses[1, 0:3] + R1 @ tic

    def _drop_oldest(self):
        """The oldest frame leaves the window lists and the states move up."""
        self.frames.pop(0)
        self.intervals.pop(0)
        self.preint.pop(0)
        if self.bias_relinearize is not None:
            self._imu_stale = True
        self.poses[:-1], self.sb[:-1] = self.poses[1:].copy(), self.sb[1:].copy()

    def slide_lists(self, margin_old):
        """The window lists' side of slideWindowOld (estimator.cpp:1144-1199) or slideWindowNew (:1201-1206, the frame_count - 1
        branch of :1163-1186), behind the FeatureManager's.  A state= driver keeps only the frame numbers: the states and the
        intervals slid in the slot, and the next step pulls them."""
        if self.est is not None:
            self.frames.pop(0 if margin_old else WINDOW_SIZE - 1)
            return
        if margin_old:
            self._drop_oldest()
            return
        # the IMU samples of the newest interval are appended to the one before it
        a, b = self.intervals[WINDOW_SIZE - 2], self.intervals[WINDOW_SIZE - 1]
        merged = dict(acc0=a["acc0"], gyr0=a["gyr0"], dt=a["dt"] + b["dt"], acc=a["acc"] + b["acc"], gyr=a["gyr"] + b["gyr"])
        self.intervals[WINDOW_SIZE - 2:] = [merged]
        if self.bias_relinearize is None:
            self.preint[WINDOW_SIZE - 2:] = [synth.preintegrate(merged["acc0"], merged["gyr0"], np.zeros(3), np.zeros(3),
                                                               merged["dt"], merged["acc"], merged["gyr"], **self.noise)]
        else:
            self.preint[WINDOW_SIZE - 2:] = [None]
            self._imu_stale = True
            self._repropagate([WINDOW_SIZE - 2])
        self.frames.pop(WINDOW_SIZE - 1)
        self.poses[WINDOW_SIZE - 1], self.sb[WINDOW_SIZE - 1] = self.poses[WINDOW_SIZE].copy(), self.sb[WINDOW_SIZE].copy()

    def propagate_next_frame(self):
        """The next image on the host: its interval joins the lists and processIMU's propagation predicts its state from the newest
        one.  Returns its number.  (An initialised state= driver's next frame comes into the slot instead: begin_next_frame.)"""
        st = self.s
        f = self.next_frame
        self.next_frame += 1
        last = self.frames[-1]
        # raw samples from `last` to f (consecutive global frames unless frames were skipped: they never are here)
        iv = dict(st.imu[last])
        pre = st.preint[last]
        self.frames.append(f)
        self.intervals.append(iv)
        self.preint.append(pre)
        if self.bias_relinearize is not None:
            self._imu_stale = True
            self._repropagate([WINDOW_SIZE - 1])
            pre = self.preint[WINDOW_SIZE - 1]
        dt = pre["sum_dt"]
        i = WINDOW_SIZE - 1
        Ri = synth.quat_to_rot(self.poses[i, 3:7])
        g = np.array([0.0, 0.0, self.g_norm])
        Pi, Vi = self.poses[i, 0:3], self.sb[i, 0:3]
        self.poses[WINDOW_SIZE, 0:3] = Pi + Vi * dt - 0.5 * g * dt * dt + Ri @ pre["delta_p"]
        self.poses[WINDOW_SIZE, 3:7] = synth.quat_mul(self.poses[i, 3:7], pre["delta_q"])
        self.sb[WINDOW_SIZE, 0:3] = Vi - g * dt + Ri @ pre["delta_v"]
        self.sb[WINDOW_SIZE, 3:9] = self.sb[i, 3:9]
        return f

    def run(self):
        while self.step():
            pass
        return np.array([np.concatenate([[t], p]) for t, p in self.trajectory])

    def ground_truth(self):
        st = self.s
        return np.array([np.concatenate([[t], st.P[k], st.Q[k]])
                         for k, t in enumerate(st.times)
                         if k >= (WINDOW_SIZE if self.init_frame is None else self.init_frame)])[:len(self.trajectory)]


def ate_rmse(traj, gt):
    """Translation APE without alignment (the windows are anchored to the initial frame), RMSE in metres."""
    d = traj[:, 1:4] - gt[:, 1:4]
    return float(np.sqrt((d * d).sum(axis=1).mean()))


def read_tum(path):
    """TUM trajectory file: `stamp px py pz qx qy qz qw` per line (System.cpp:438), '#' comments allowed."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                rows.append([float(v) for v in line.replace(",", " ").split()[:8]])
    return np.array(rows, dtype=np.float64).reshape(-1, 8)


def associate(est, gt, max_diff=0.01):
    """Pair every estimated stamp with the closest ground-truth stamp not further than max_diff (one to one, in time
    order) — the association of `evo_ape tum` (README.md:169 of the reference's assignment 17)."""
    ti, tj = est[:, 0], gt[:, 0]
    j = np.clip(np.searchsorted(tj, ti), 1, len(tj) - 1)
    j = np.where(np.abs(tj[j - 1] - ti) <= np.abs(tj[j] - ti), j - 1, j)
    ok = np.abs(tj[j] - ti) <= max_diff
    # one to one: keep the first estimate claiming a ground-truth sample
    _, first = np.unique(np.where(ok, j, -1), return_index=True)
    keep = np.zeros(len(ti), dtype=bool)
    keep[first] = True
    keep &= ok
    return np.nonzero(keep)[0], j[keep]


def umeyama_se3(x, y):
    """Rotation R and translation t minimising sum |R x_k + t - y_k|^2 (Umeyama 1991, no scale): `evo_ape -a`."""
    mx, my = x.mean(axis=0), y.mean(axis=0)
    S = (y - my).T @ (x - mx) / len(x)
    U, _, Vt = np.linalg.svd(S)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    return R, my - R @ mx


def ape_stats(est, gt, align=True, max_diff=0.01):
    """Translation APE statistics as `evo_ape tum gt est -va` prints them (rmse, mean, median, std, min, max, sse)."""
    ie, ig = associate(est, gt, max_diff)
    x, y = est[ie, 1:4], gt[ig, 1:4]
    if align:
        R, t = umeyama_se3(x, y)
        x = x @ R.T + t
    e = np.linalg.norm(x - y, axis=1)
    return {"rmse": float(np.sqrt((e * e).mean())), "mean": float(e.mean()), "median": float(np.median(e)),
            "std": float(e.std()), "min": float(e.min()), "max": float(e.max()), "sse": float((e * e).sum()),
            "pairs": int(len(e))}


def write_tum(path, traj):
    with open(path, "w") as f:
        for row in traj:
            f.write(" ".join("%.9f" % v for v in row) + "\n")
