"""B stream drivers advanced in lockstep, with the frame's two heavy calls batched over them: one vio_batch_solve for every window's
Problem::Solve(10) and one vio_marg_compute_batch (include/vio_marg.h) for every window's MargOldFrame / MargNewFrame.

    drivers = [StreamDriver(hip, SyntheticStream(seed=s), ctx_kwargs=dict(stream=stream)) for s in seeds]   # contexts on one stream
    trajectories = run_batched(drivers, vio.load_marg().create(stream=stream))

Each driver keeps its own bookkeeping (FeatureManager, slide, the next frame) exactly as StreamDriver.step does it; what changes is
that the marginalisation takes the re-anchored window's host arrays directly (as MargOldFrame builds a fresh Problem from para_*,
estimator.cpp:693-829) instead of reloading the context and calling vio_marginalize.  Results agree with StreamDriver.run to the
rounding of the two marginalisation tails.  Drivers created with features=(fm_handle, slot) keep that bookkeeping in the slots of one
fm.FmHandle, and the frame's FeatureManager work is then one batched call per step for all of them.
"""
import numpy as np

from .capi import MARG_OLD, MARG_SECOND_NEW, WINDOW_SIZE
from .stream import (FM_BACK, FM_BACK_SHIFT_DEPTH, FM_FRONT, anchor_gauge, est_flush, est_init_apply, est_relinearize, fm_add, fm_init_depths,
                     fm_remove, fm_set_depths, fm_slide, fm_tracks, fm_windows)


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
    without a threshold take part in neither."""
    est, fm = drivers[0].est, drivers[0].fm
    if est is not None:
        est_relinearize(drivers)    # (state=dict(relinearize=): one relinearize_batch in front of the window call)
        for d, win in zip(drivers, est.window_batch([d.est_slot for d in drivers])):
            d.pull_window(win)
    if fm is not None:
        loaded = fm_windows(drivers, True)
        for d, (w, _) in zip(drivers, loaded):
            d.ctx.load(w)
    else:
        for d in drivers:
            d.ensure_depths()
        loaded = []
        for d in drivers:
            w, ids = d.window_arrays()
            d.ctx.load(w)
            loaded.append((w, ids))
    reps = drivers[0].lib.batch_solve([d.ctx for d in drivers], 10)
    jobs = []
    solved = [d.ctx.get_window() for d in drivers]
    if est is not None:             # double2vector + failureDetection of every window in one call
        for d, r in zip(drivers, est.update_batch([(d.est_slot, s[0], s[1], d.ext, True) for d, s in zip(drivers, solved)])):
            d.apply_update(r)
    invds = [d.ctx.get_landmarks() for d in drivers]
    if fm is not None:
        fm_set_depths(drivers, invds)
    bad = _flagged(drivers, loaded)
    for d, (w, ids), rep, (poses, sb, _), invd in zip(drivers, loaded, reps, solved, invds):
        if d.prior is not None:      # estimator.cpp:1040-1049: b/err prior come back updated, H/Jt stay
            b, e = d.ctx.get_prior()
            d.prior = dict(d.prior, b=b[:156].copy(), err=e.copy())
        if est is None:
            d.poses, d.sb = anchor_gauge(w.poses, poses, sb)
        if fm is None:
            for l, v in zip(ids, invd):
                d.depth[l] = 1.0 / v
        newest = d.frames[WINDOW_SIZE]
        d.trajectory.append((d.s.times[newest], d.poses[WINDOW_SIZE].copy()))
        d.reports.append(rep)
        second_new = d.frames[WINDOW_SIZE - 1]
        margin_old = not (d.nonkey_every and second_new % d.nonkey_every == d.nonkey_every - 1)
        kind = MARG_OLD if margin_old else MARG_SECOND_NEW
        d.flags.append(kind)
        w2 = None if fm is not None else d.window_arrays()[0]       # the re-anchored states (estimator.cpp:1086-1102)
        jobs.append((kind, w2, d.prior))
    if fm is not None:
        jobs = [(kind, w2, prior) for (kind, _, prior), (w2, _) in zip(jobs, fm_windows(drivers, False))]
    priors = marg.compute_batch(jobs)
    if bad:                         # removeOutlier + removeFailures, before the slides
        for d, ids in bad:
            d.record_rejected(ids)
        fm_remove([d for d, _ in bad], [ids for _, ids in bad])
    more = []
    if est is not None:             # slideWindow, then processIMU and the headers of the next frame, one call each
        for d, p in zip(drivers, priors):
            d.prior = p
            more.append(d.next_frame < d.s.n_frames)
        go = [(d, kind) for d, m, (kind, _, _) in zip(drivers, more, jobs) if m]
        if go:
            slid = est.slide_batch([(d.est_slot, kind, True) for d, kind in go])
            if fm is not None:
                _fm_slide_group(go, [(r["marg_R"], r["marg_P"], r["new_R"], r["new_P"]) if kind == MARG_OLD else None for (_, kind), r in zip(go, slid)])
            for (d, kind), r in zip(go, slid):
                d.apply_slide(r, kind == MARG_OLD, fm is not None)
            begun = [d.begin_next_frame() for d, _ in go]
            est.imu_batch([b[1] for b in begun])
            est.image_batch([b[2] for b in begun])
            if fm is not None:
                fm_add([d for d, _ in go], [b[0] for b in begun])
            else:
                for (d, _), b in zip(go, begun):
                    d.add_frame_observations(b[0])
        return more
    if fm is not None:
        for d, p in zip(drivers, priors):
            d.prior = p
            more.append(d.next_frame < d.s.n_frames)
        go = [(d, kind) for d, m, (kind, _, _) in zip(drivers, more, jobs) if m]
        if go:
            _fm_slide_group(go, [d.slide_mats() if kind == MARG_OLD else None for d, kind in go])
            for d, kind in go:
                if kind == MARG_OLD:
                    d.slide_window_old(fm_done=True)
                else:
                    d.slide_window_new(fm_done=True)
                d.take_next_frame(observe=False)
            fm_add([d for d, _ in go], [d.frames[-1] for d, _ in go])
        return more
    for d, p, (kind, _, _) in zip(drivers, priors, jobs):
        d.prior = p
        if d.next_frame >= d.s.n_frames:
            more.append(False)
            continue
        if kind == MARG_OLD:
            d.slide_window_old()
        else:
            d.slide_window_new()
        d.take_next_frame()
        more.append(True)
    return more


def _flagged(drivers, loaded):
    """(driver, feature ids the residual query condemns) of every driver created with outlier_px: FeaturePerId::is_outlier /
    solve_flag = 2 from the solved states the contexts hold, on the windows they were loaded with.  One batch_residuals per distinct
    threshold, flags only."""
    out = {}
    for px in sorted({d.outlier_px for d in drivers if d.outlier_px is not None}):
        who = [i for i, d in enumerate(drivers) if d.outlier_px == px]
        res = drivers[0].lib.batch_residuals([drivers[i].ctx for i in who], [loaded[i][0] for i in who], outlier_px=px, outputs=("flags",))
        for i, r in zip(who, res):
            ids = loaded[i][1]
            out[i] = [ids[k] for k in np.nonzero(r["flags"] & 7)[0]]
    return [(drivers[i], out[i]) for i in sorted(out)]


def _fm_slide_group(go, mats):
    """The slot side of the frame's slides, both kinds in one slide_batch: go: (driver, marginalisation flag); mats: the four arrays
    of slideWindowOld for a MARG_OLD driver."""
    fm_slide([d for d, _ in go], [FM_BACK_SHIFT_DEPTH if kind == MARG_OLD else FM_FRONT for _, kind in go], mats)


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
    and one init_apply_batch for its successes.  Returns the number of rounds."""
    pending = [d for d in drivers if not d.initialized]
    rounds = 0
    while pending:
        groups = {}
        for d in pending:
            groups.setdefault(_init_group_key(d), []).append(d)
        for group in groups.values():
            est = group[0].est is not None
            if est:                 # the slots' feeding: the window in the first round, the last round's failures afterwards
                est_flush(group)
            if group[0].fm is not None:
                won = _init_round_fm(group, est)
            else:
                reqs = [d.init_request() for d in group]
                res = group[0].init_align([r[0] for r in reqs], [r[1] for r in reqs])
                won = [(d, r) for d, (item, _), r in zip(group, reqs, res) if d.init_apply(item, r, est_batched=est)]
            if est and won:
                est_init_apply([d for d, _ in won], [r for _, r in won])
        pending = [d for d in pending if not d.initialized]
        rounds += 1
    return rounds


def _init_round_fm(group, est_batched=False):
    """One round of a group whose FeatureManagers live in slots (features=): one tracks_batch gives every window's sfm_f, the tries
    run as ever, and their outcomes end in one init_depth_batch for the successes and one slide_batch (BACK) and one add_batch for
    the failures (StreamDriver.init_apply does each driver's own part)."""
    sfm = bool(group[0].initialize.get("sfm"))
    tracks = fm_tracks(group) if sfm else [None] * len(group)
    reqs = [d.init_request(tr) for d, tr in zip(group, tracks)]
    res = group[0].init_align([r[0] for r in reqs], [r[1] for r in reqs])
    won, lost = [], []
    for d, (item, _), r in zip(group, reqs, res):
        (won if d.init_apply(item, r, fm_batched=True, est_batched=est_batched) else lost).append((d, item, r))
    if won:
        fm_init_depths([d for d, _, _ in won], [item for _, item, _ in won], [float(r["s"]) for _, _, r in won])
    if lost:
        ds = [d for d, _, _ in lost]
        fm_slide(ds, [FM_BACK] * len(ds))
        fm_add(ds, [d.frames[-1] for d in ds])
        aif = [d for d in ds if d.aif is not None]
        for d, tr in zip(aif, fm_tracks(aif) if aif else []):
            d._aif_push(len(d.frames) - 1, slide=d.s.times[d._fm_gone], tracks=tr)
    return [(d, r) for d, _, r in won]


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
