"""The inputs of the extrinsic rotation calibration's tests at its limits (tests/test_exrot_limits_inputs_cpu.py proves on the numpy
restatement alone that each is what it claims to be, tests/test_gpu_exrot_limits.py runs them on the device).  No tests in here, no
GPU and no library: numpy over tests/exrot_reference.py and tests/sfm_reference.py.

Stage 1 (k_exrot_pairs: thread t owns tracks [t C, (t + 1) C), C = ceil(nt / 256)):
    cut(n)                  the first n tracks of one F = 2 window of 4580 tracks: n tracks are n correspondences
    sparse(nt)              F = 3, nt tracks: only every C-th run holds correspondences of pair 0, two of them, at its first and its
                            last track; every other track is a length-2 track of pair 1
    ends()                  F = 4, 4096 tracks: pair 0's correspondences all in the last run, pair 1's all in the first, pair 2's between
    unequal(counts)         F = 11: a make_window window whose tracks are cut in two at some pairs so that those pairs keep exactly
                            0, 8 or 9 correspondences and the others stay full; no track is dropped, so no other pair thins
    degenerate()            F = 4, finite points whose fit is not finite: every frame-0 point of pair 0 is (0.125, 0.25)
Stage 2 (k_exrot_solve), all with exact Rc[k] = ric^T R_imu[k] ric:
    branches(i)             F = 32, rotations of 130 + 1.5 k degrees about axes cycling near x, y, z: ric of 2.8 rad near x, y, z (i = 0,
                            1, 2) and of 0.6 rad (i = 3): every rot_to_quat call leaves the trace branch
    huber_determined()      F = 17, the first three pairs 2 degrees about different axes (ric determined from step 2 on whatever step 1
                            gave), then 20 .. 170 degrees with delta_q 20 and 60 degrees off in five pairs
    knee()                  F = 31, all rotations <= 100 degrees, one delta_q 4.9 and one 5.1 degrees off
    stage2_batch()          96 windows cycling F over 2, 3, 11, 17, 31, 32: runs of consecutive pairs of the fixtures above
    branch_table(...)       which rot_to_quat branch each of k_exrot_solve's four call sites takes at every step
    perturb_stage2(...)     every entry of Rc and delta_q one ulp in a random direction
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exrot_reference as xr  # noqa: E402
import sfm_reference as sr  # noqa: E402

PX = 1.0 / 460.0
NT = 256                                            # k_exrot_pairs' workgroup
MAX_TRACKS = 4096
CUT_SIZES = (63, 64, 65, 255, 256, 257, 512, 513, 4096)
SPARSE_SIZES = (513, 4096)
FULL = -1
UNEQUAL = (FULL, 0, FULL, 8, FULL, 9, FULL, FULL, FULL, FULL)
BATCH_F = (2, 3, 11, 17, 31, 32)
NO_HUBER = dict(huber_deg=1e3)
SITES = ("Rc", "Rimu", "Rc_g", "ric")
BRANCH_NAMES = ("trace", "x", "y", "z")
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def run_size(nt):
    """C of k_exrot_pairs: the tracks one thread owns."""
    return (nt + NT - 1) // NT


# ---- stage 1 -------------------------------------------------------------------------------------------
def first_tracks(item, n):
    return dict(item, start_frame=item["start_frame"][:n], obs_offset=item["obs_offset"][:n + 1], pts=item["pts"][:item["obs_offset"][n]])


def source(F):
    """One window of F frames with more than 4096 tracks (30000 points, 8 degrees a frame, 0.1 px)."""
    return _cached(("source", F), lambda: xr.make_window(4, 8, F=F, noise=0.1 * PX, n_points=30000)[0])


def cut(n):
    return first_tracks(source(2), n)


def compose(src, parts):
    """The window of the tracks (j, lo, hi) in that order: frames lo .. hi of src's track j."""
    sf, off, pts = np.asarray(src["start_frame"]), np.asarray(src["obs_offset"]), np.asarray(src["pts"]).reshape(-1, 2)
    out_sf, out_off, out_pts = [], [0], []
    for j, lo, hi in parts:
        assert sf[j] <= lo <= hi <= sf[j] + (off[j + 1] - off[j]) - 1, (j, lo, hi)
        out_sf.append(lo)
        out_pts.append(pts[off[j] + lo - sf[j]:off[j] + hi - sf[j] + 1])
        out_off.append(out_off[-1] + hi - lo + 1)
    return dict(src, start_frame=np.array(out_sf, dtype=np.int32), obs_offset=np.array(out_off, dtype=np.int64),
                pts=np.concatenate(out_pts).reshape(-1, 2) if out_pts else np.zeros((0, 2)))


def _whole(src):
    """src's tracks seen in every frame."""
    sf, off = np.asarray(src["start_frame"]), np.asarray(src["obs_offset"])
    return np.nonzero((sf == 0) & (off[1:] - off[:-1] == src["n_frames"]))[0]


def sparse(nt):
    """Tracks seen in all three frames of source(3), used once each: run r = 0, C, 2 C, .. (of C tracks) starts with a whole track
    (pairs 0 and 1) and ends with one cut to frames 0 .. 1 (pair 0 only); every other track is cut to frames 1 .. 2 (pair 1 only)."""
    def make():
        src, C = source(3), run_size(nt)
        whole = _whole(src)
        assert len(whole) >= nt
        parts = []
        for j in range(nt):
            run, pos = divmod(j, C)
            last = min(nt, (run + 1) * C) - 1 - run * C
            if run % C == 0 and pos == 0:
                parts.append((whole[j], 0, 2))
            elif run % C == 0 and pos == last:
                parts.append((whole[j], 0, 1))
            else:
                parts.append((whole[j], 1, 2))
        return compose(src, parts)
    return _cached(("sparse", nt), make)


def ends():
    """4096 tracks of source(4), C = 16: the first run holds 16 tracks of frames 1 .. 2, the last run 16 tracks of frames 0 .. 1 and
    every run between tracks of frames 2 .. 3."""
    def make():
        src, C = source(4), run_size(MAX_TRACKS)
        whole = _whole(src)
        assert len(whole) >= MAX_TRACKS
        parts = [(whole[j], 1, 2) if j < C else ((whole[j], 0, 1) if j >= MAX_TRACKS - C else (whole[j], 2, 3)) for j in range(MAX_TRACKS)]
        return compose(src, parts)
    return _cached("ends", make)


def runs_with(item, k):
    """How many correspondences of pair k each of the 256 threads owns, and the positions inside its run where they sit."""
    sf, off = np.asarray(item["start_frame"]), np.asarray(item["obs_offset"])
    nt = len(sf)
    C = run_size(nt)
    cov = (sf <= k) & (sf + (off[1:] - off[:-1]) - 1 >= k + 1)
    counts = np.array([cov[t * C:min(nt, (t + 1) * C)].sum() for t in range(NT)])
    where = [np.nonzero(cov[t * C:min(nt, (t + 1) * C)])[0].tolist() for t in range(NT)]
    return counts, where


def unequal_source():
    return _cached("unequal_source", lambda: xr.make_window(1, 8, noise=0.1 * PX, n_points=500)[0])


def unequal(counts=UNEQUAL):
    """unequal_source() (F = 11, 500 points, 8 degrees a frame, 0.1 px: more than 60 correspondences a pair) with pair k left counts[k] correspondences (FULL: all of
    them): the tracks covering the pair beyond its first counts[k] are cut in two between frames k and k + 1, and both halves stay as
    tracks in the track's place (a half may be a single observation, which covers no pair)."""
    def make():
        src = unequal_source()
        sf, off = np.asarray(src["start_frame"]), np.asarray(src["obs_offset"])
        seen = [0] * len(counts)
        parts = []
        for j in range(len(sf)):
            lo, hi = int(sf[j]), int(sf[j] + off[j + 1] - off[j] - 1)
            for k in range(lo, hi):
                if counts[k] != FULL:
                    seen[k] += 1
                    if seen[k] > counts[k]:
                        parts.append((j, lo, k))
                        lo = k + 1
            parts.append((j, lo, hi))
        return compose(src, parts)
    return _cached(("unequal", tuple(counts)), make)


DEGENERATE_POINT = (0.125, 0.25)                    # exactly representable: the centroid is exact and every distance to it is 0
INEXACT_POINT = (0.1, 0.2)                          # not used: see test_exrot_limits_inputs_cpu.py


def degenerate_base():
    return _cached("degenerate_base", lambda: xr.make_window(1, 8, F=4, noise=0.1 * PX)[0])


def degenerate(point=DEGENERATE_POINT):
    """degenerate_base() with every frame-0 point of the tracks covering pair 0 at `point`: Hartley's mean distance of pair 0's first
    point set is 0, its scale infinite and the fit NaN, from finite inputs.  Frame 0 belongs to pair 0 only."""
    item = degenerate_base()
    sf, off = np.asarray(item["start_frame"]), np.asarray(item["obs_offset"])
    pts = np.array(item["pts"], dtype=np.float64).reshape(-1, 2)
    pts[off[:-1][sf == 0]] = point
    return dict(item, pts=pts)


# ---- stage 2 -------------------------------------------------------------------------------------------
def _axis(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _rot(axis, deg):
    return sr.exp_so3(_axis(axis) * np.radians(deg))


def stage2_item(ric, Rimu, off=None):
    """(item, Rc): Rc[k] = ric^T R_imu[k] ric, delta_q[k] the quaternion of R_imu[k] (of R_imu[k] off[k] where off names the pair)."""
    Rc = np.array([(ric.T @ R) @ ric for R in Rimu])
    dq = np.array([sr.rot_to_quat(R @ (off or {}).get(k, np.eye(3))) for k, R in enumerate(Rimu)])
    return dict(n_frames=len(Rimu) + 1, delta_q=dq), Rc


NEAR_AXES = ((1.0, 0.08, -0.05), (-0.06, 1.0, 0.07), (0.05, -0.09, 1.0))
BRANCH_RIC = ((2.8, NEAR_AXES[0]), (2.8, NEAR_AXES[1]), (2.8, NEAR_AXES[2]), (0.6, (0.5, -0.6, 0.62)))


def branches(i):
    def make():
        ang, ax = BRANCH_RIC[i]
        ric = sr.exp_so3(_axis(ax) * ang)
        return stage2_item(ric, [_rot(NEAR_AXES[k % 3], 130.0 + 1.5 * k) for k in range(xr.MAX_FRAMES - 1)]) + (ric,)
    return _cached(("branches", i), make)


RIC_06 = (0.6, (0.3, -0.7, 0.65))
HUBER_DEG = (2, 2, 2, 20, 35, 50, 65, 80, 95, 110, 125, 140, 150, 160, 170, 45)
HUBER_AXES_SEED = 6                                 # chosen on the CPU: all four branches at the Rc, Rimu and Rc_g sites, z at ric's
HUBER_OFF = {4: ((0, 1, 0), 20.0), 7: ((1, 0, 0), 60.0), 9: ((0, 0, 1), 20.0), 11: ((0, 1, 1), 60.0), 13: ((1, 1, 0), 20.0)}


def _varied_axes(n, seed):
    rng = np.random.RandomState(seed)
    return [NEAR_AXES[k] if k < 3 else rng.normal(size=3) for k in range(n)]


def huber_determined():
    def make():
        ric = sr.exp_so3(_axis(RIC_06[1]) * RIC_06[0])
        axes = _varied_axes(len(HUBER_DEG), HUBER_AXES_SEED)
        return stage2_item(ric, [_rot(axes[k], d) for k, d in enumerate(HUBER_DEG)], {k: _rot(*v) for k, v in HUBER_OFF.items()}) + (ric,)
    return _cached("huber", make)


KNEE_PAIRS = {20: ((0, 1, 0), 5.1), 26: ((1, 0, 0), 4.9)}          # pair: the axis and the angle its delta_q is off by


def knee():
    def make():
        ric = sr.exp_so3(_axis(RIC_06[1]) * RIC_06[0])
        deg = [2, 2, 2] + [20.0 + 80.0 * ((7 * k) % 27) / 26.0 for k in range(27)]
        axes = _varied_axes(len(deg), 12)
        return stage2_item(ric, [_rot(axes[k], d) for k, d in enumerate(deg)], {k: _rot(*v) for k, v in KNEE_PAIRS.items()}) + (ric,)
    return _cached("knee", make)


def branch_of(R):
    """sfm_reference.rot_to_quat's branch for R: 0 the trace, 1 + i the largest diagonal entry i; and how far R is from the nearest
    other decision (the trace from 0, the compared diagonal entries from each other)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        return 0, abs(t)
    i = 1 if R[1, 1] > R[0, 0] else 0
    m = min(abs(t), abs(R[1, 1] - R[0, 0]), abs(R[2, 2] - R[i, i]))
    return (3 if R[2, 2] > R[i, i] else 1 + i), m


def branch_table(Rc, dq, out):
    """(table, margin): the branch of each of k_exrot_solve's four rot_to_quat calls at every step, (P, 4) over SITES, from the
    restatement's result `out` of (Rc, dq); margin as branch_of's."""
    Rc, dq = np.asarray(Rc).reshape(-1, 3, 3), np.asarray(dq).reshape(-1, 4)
    tab, mar = [], []
    for k in range(len(Rc)):
        Rimu = sr.quat_to_rot(dq[k])
        ric = out["step_ric"][k - 1] if k else np.eye(3)
        rows = [branch_of(Rc[k]), branch_of(Rimu), branch_of((ric.T @ Rimu) @ ric), branch_of(out["step_ric"][k])]
        tab.append([r[0] for r in rows])
        mar.append([r[1] for r in rows])
    return np.array(tab), np.array(mar)


def distances(Rc, dq, out):
    """The angular distance, in degrees, that gives each pair's Huber weight (with the ric of the step before)."""
    d = []
    for k in range(len(Rc)):
        ric = out["step_ric"][k - 1] if k else np.eye(3)
        d.append(xr.angular_distance_deg(sr.rot_to_quat(Rc[k]), sr.rot_to_quat((ric.T @ sr.quat_to_rot(dq[k])) @ ric)))
    return np.array(d)


def _ulp(a, rng):
    a = np.asarray(a, dtype=np.float64)
    return np.where(rng.rand(*a.shape) < 0.5, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))


def perturb_stage2(item, Rc, rng):
    """(item, Rc) with every entry of Rc and of delta_q moved by one ulp in a random direction."""
    return dict(item, delta_q=_ulp(item["delta_q"], rng)), _ulp(Rc, rng)


def stage2_sources():
    return [branches(i)[:2] for i in range(4)] + [huber_determined()[:2], knee()[:2]]


def stage2_batch():
    """96 (item, Rc): window i has F = BATCH_F[i % 6] and is a run of F - 1 consecutive pairs of source (i // 6) % 6 of
    stage2_sources(), from its pair 5 i on, going round at the source's end."""
    def make():
        src, out = stage2_sources(), []
        for i in range(96):
            item, Rc = src[(i // 6) % len(src)]
            idx = (5 * i + np.arange(BATCH_F[i % 6] - 1)) % len(Rc)
            n = len(idx)
            out.append((dict(n_frames=n + 1, delta_q=item["delta_q"][idx].copy()), Rc[idx].copy()))
        return out
    return _cached("batch", make)


# ---- the fixtures with their restatement and its spread ---------------------------------------------------
PAIR_KEYS = ("n_corres", "front", "choice", "det_flip")
STEP_KEYS = ("step_q", "step_ric", "sigma", "huber", "q", "ric")
N_PERTURB = 3
STAGE1 = dict([("cut%d" % n, lambda n=n: cut(n)) for n in CUT_SIZES] + [("sparse%d" % n, lambda n=n: sparse(n)) for n in SPARSE_SIZES] +
              [("ends", ends), ("unequal", unequal), ("unequal_rev", lambda: unequal(UNEQUAL[::-1])), ("degenerate_base", degenerate_base)])
# name: (builder, config, the first step index from which ric is determined by the inputs)
STAGE2 = dict([("branches%d" % i, (lambda i=i: branches(i), NO_HUBER, 2)) for i in range(4)] +
              [("huber", (huber_determined, {}, 1)), ("knee", (knee, {}, 1))])


def _spread(runs, ref, keys):
    return {k: np.max([np.nan_to_num(np.abs(p[k] - ref[k])) for p in runs], axis=0) for k in keys}


def stage1(name):
    """(item, restatement, spread) of a STAGE1 window, computed once: the spread over N_PERTURB one-ulp perturbations of the points,
    under which every discrete outcome must stay (a window where one does not would not be a fixture)."""
    def make():
        item = STAGE1[name]()
        ref = xr.exrot(item)
        rng = np.random.RandomState(7)
        runs = [xr.exrot(xr.perturb_ulp(item, rng)) for _ in range(N_PERTURB)]
        for p in runs:
            assert (p["status"], p["step"], p["pairs"]["status"]) == (ref["status"], ref["step"], ref["pairs"]["status"]), name
            for k in PAIR_KEYS:
                assert np.array_equal(p["pairs"][k], ref["pairs"][k]), (name, k)
        sp = _spread(runs, ref, STEP_KEYS)
        sp["Rc"] = _spread([p["pairs"] for p in runs], ref["pairs"], ("Rc",))["Rc"]
        return item, ref, sp
    return _cached(("stage1", name), make)


def determined(P, first):
    """(P, 4) over SITES: the branch decisions that the inputs determine.  Rc and Rimu always; ric from step index `first` on; Rc_g at
    step index 0 (from the identity) and where the ric of the step before is determined."""
    m = np.ones((P, 4), dtype=bool)
    m[:first, 3] = False
    m[1:first + 1, 2] = False
    return m


def stage2(name):
    """A STAGE2 window, computed once: a dict of item, Rc, true ric, cfg, first, the restatement `ref`, the perturbed restatements
    `runs` (N_PERTURB of perturb_stage2), their spread `sp`, the branch table and its margins.  (status, step) and every determined
    branch decision must stay under the perturbations."""
    def make():
        build, cfg, first = STAGE2[name]
        item, Rc, ric = build()
        ref = xr.calibrate(Rc, item["delta_q"], cfg)
        table, margin = branch_table(Rc, item["delta_q"], ref)
        det = determined(len(Rc), first)
        rng = np.random.RandomState(7)
        runs = []
        for _ in range(N_PERTURB):
            it2, Rc2 = perturb_stage2(item, Rc, rng)
            p = xr.calibrate(Rc2, it2["delta_q"], cfg)
            assert (p["status"], p["step"]) == (ref["status"], ref["step"]), name
            assert np.array_equal(branch_table(Rc2, it2["delta_q"], p)[0][det], table[det]), name
            runs.append(dict(p, Rc=Rc2, delta_q=it2["delta_q"]))
        return dict(item=item, Rc=Rc, ric=ric, cfg=cfg, first=first, ref=ref, runs=runs, sp=_spread(runs, ref, STEP_KEYS), table=table,
                    margin=margin, determined=det)
    return _cached(("stage2", name), make)


def coverage(name):
    """The branch coverage of a STAGE2 window: per site, the sorted branches among its determined decisions."""
    fx = stage2(name)
    return {s: sorted(set(fx["table"][fx["determined"][:, i], i].tolist())) for i, s in enumerate(SITES)}


def coverage_table(names=None):
    lines = ["%-10s " % "window" + " ".join("%-22s" % s for s in SITES)]
    for n in names or list(STAGE2):
        c = coverage(n)
        lines.append("%-10s " % n + " ".join("%-22s" % ",".join(BRANCH_NAMES[b] for b in c[s]) for s in SITES))
    return "\n".join(lines)
