"""B stream drivers advanced in lockstep, with the frame's two heavy calls batched over them: one vio_batch_solve for every window's
Problem::Solve(10) and one vio_marg_compute_batch (include/vio_marg.h) for every window's MargOldFrame / MargNewFrame.

    drivers = [StreamDriver(hip, SyntheticStream(seed=s), ctx_kwargs=dict(stream=stream)) for s in seeds]   # contexts on one stream
    trajectories = run_batched(drivers, vio.load_marg().create(stream=stream))

The frame and the INITIAL round are stream.step_group's and stream.init_round's, which StreamDriver.step runs for a group of one; what
changes is BatchedCalls: one solve for the group, and the marginalisation takes the re-anchored window's host arrays directly (as MargOldFrame builds a fresh Problem from para_*,
estimator.cpp:693-829) instead of reloading the context and calling vio_marginalize.  Results agree with StreamDriver.run to the
rounding of the two marginalisation tails.  Drivers created with features=(fm_handle, slot) keep that bookkeeping in the slots of one
fm.FmHandle, and the frame's FeatureManager work is then one batched call per step for all of them.
"""
import numpy as np

from .stream import init_round, step_group


def _check(drivers):
    for i, d in enumerate(drivers):
        if d.outlier_px is not None and (d.fm is None or not hasattr(d.fm, "remove_batch")):
            raise ValueError("run_batched: driver %d was created with outlier_px and without features= on a handle with remove_batch "
                             "(the residual query is batched here for FeatureManagers in slots only)" % i)
        if d.bias_relinearize is not None:
            raise ValueError("run_batched: driver %d was created with bias_relinearize (not batched here)" % i)
    libs = {id(d.lib) for d in drivers}
    if len(libs) > 1:
        raise ValueError("run_batched: the drivers' contexts belong to different libraries")
    streams = {d.ctx.get_stream() for d in drivers}
    if len(streams) > 1:
        raise ValueError("run_batched: the drivers' contexts must share one stream (ctx_kwargs=dict(stream=...))")
    if len({id(d.est) for d in drivers}) > 1:
        raise ValueError("run_batched: the drivers must share one estimator-state handle (state=(handle, slot)), or none has one")
    if drivers and drivers[0].est is not None and len({d.est_slot for d in drivers}) != len(drivers):
        raise ValueError("run_batched: two drivers share an estimator-state slot")
    if len({id(d.fm) for d in drivers}) > 1:
        raise ValueError("run_batched: the drivers must share one FeatureManager handle (features=(handle, slot)), or none has one")
    if drivers and drivers[0].fm is not None and len({d.fm_slot for d in drivers}) != len(drivers):
        raise ValueError("run_batched: two drivers share a FeatureManager slot")


def step_batched(drivers, marg):
    """One frame of every driver in `drivers` (all not finished).  Returns, per driver, whether it has another frame.  Drivers
    created with state= share a handle (_check): the frame then makes one window, one update, one slide and one processIMU call (and
    one for the headers) for all of them.  Drivers created with features= share a handle too: the frame then makes one export, one
    set-depth, one second export, one slide and one add call for all of them.  Where a driver was created with
    state=dict(relinearize=), one relinearize_batch goes in front of the window call.  Where drivers were created with outlier_px
    (features= too, _check), the frame makes one batched residual query per distinct threshold over them behind the solve, flags only,
    and one remove_batch of the flagged landmarks' feature ids behind the marginalisation and in front of the slides; the drivers
    without a threshold take part in neither.  The frame itself is stream.step_group's."""
    return step_group(drivers, BatchedCalls(marg))


class BatchedCalls:
    """The frame's three heavy calls, once for the group (stream.OwnContexts issues them per driver): vio_batch_solve, one
    batch_residuals per distinct threshold, vio_marg_compute_batch on the re-anchored windows' host arrays."""

    def __init__(self, marg):
        self.marg = marg

    def solve(self, drivers):
        return drivers[0].lib.batch_solve([d.ctx for d in drivers], 10)

    def flags(self, drivers, windows):
        out = [None] * len(drivers)
        for px in sorted({d.outlier_px for d in drivers if d.outlier_px is not None}):
            who = [i for i, d in enumerate(drivers) if d.outlier_px == px]
            res = drivers[0].lib.batch_residuals([drivers[i].ctx for i in who], [windows[i] for i in who], outlier_px=px, outputs=("flags",))
            for i, r in zip(who, res):
                out[i] = r["flags"]
        return out

    def marginalize(self, drivers, jobs):
        return self.marg.compute_batch(jobs)


def _init_group_key(d):
    """What one alignment call shares across its windows: the extrinsic translation (TIC[0]), G, the IMU noise of the re-propagation,
    the aligner, the SfM, the extrinsic rotation calibration, the all_image_frame handle (all_frames), the FeatureManager handle (features), the estimator-state handle (state) and the device the group's handles are created on.  Drivers that differ in any of them are aligned in separate calls."""
    noise = tuple(sorted((k, float(v)) for k, v in d.noise.items()))
    sfm = d.initialize.get("sfm")
    cal = d.initialize.get("calibrate_ric")
    cal = id(cal) if callable(cal) else (tuple(sorted(cal.items())) if isinstance(cal, dict) else bool(cal))
    return (tuple(float(v) for v in d.ext[0:3]), float(d.g_norm), noise, id(d.initialize.get("aligner")),
            id(sfm) if callable(sfm) else bool(sfm), cal, int(d.ctx.cfg.device), id(d.aif), id(d.fm), id(d.est))


def initialize_batched(drivers):
    """The initialisation tries of every driver created with `initialize` that is not initialised yet, in batched rounds: each round
    makes one alignment call (InitHandle.initialize_batch: one gyro launch, one re-propagation, one align launch) for every group of
    drivers still trying that share an extrinsic, G, IMU noise and aligner (usually one group), then applies each outcome as
    StreamDriver.ensure_initialized does.  Drivers created with `sfm` get their camera poses from one SfM call per group and round
    (SfmHandle.sfm_batch) in front of the alignment call, and drivers created with `calibrate_ric` their camera-IMU rotation from one
    calibration call per group and round (ExrotHandle.exrot_batch) in front of that.  Drivers created with `all_frames` take the try
    from their resident all_image_frame slots: aif.initialize_from_frames' four calls per group and round in the alignment call's
    place.  Drivers created with a `state` entry live in estimator-state slots: their initial feeding is one call per step for the
    group (est_flush), and every round then makes one slide_batch, one imu_batch and one image_batch for the last round's failures
    and one init_apply_batch for its successes.  The round itself is stream.init_round's.  Returns the number of rounds."""
    pending = [d for d in drivers if not d.initialized]
    rounds = 0
    while pending:
        groups = {}
        for d in pending:
            groups.setdefault(_init_group_key(d), []).append(d)
        for group in groups.values():
            init_round(group)
        pending = [d for d in pending if not d.initialized]
        rounds += 1
    return rounds


def run_batched(drivers, marg):
    """Run every driver to the end of its stream (StreamDriver.run, batched).  Returns each driver's trajectory as StreamDriver.run
    does.  marg: a MargHandle on the contexts' device and stream.  Drivers created with `initialize` first run their tries in batched
    rounds (initialize_batched); the others start at once."""
    drivers = list(drivers)
    _check(drivers)
    initialize_batched(drivers)
    active = list(drivers)
    while active:
        more = step_batched(active, marg)
        active = [d for d, m in zip(active, more) if m]
    return [np.array([np.concatenate([[t], p]) for t, p in d.trajectory]) for d in drivers]
