"""The window solver off vio_default_config: the windows, the configurations and the call sequences of tests/test_gpu_config.py,
with no GPU in them.  tests/test_config_cases_cpu.py asserts on the oracle alone what the GPU file assumes of every case (its
conditioning, that it differs from the default, Huber's inliers, Tukey's information); tests/test_gpu_config.py runs the device.

Two kinds of case are left out on purpose:
  - Huber with an edge beyond delta: rho' + 2 rho'' e2 is zero in exact arithmetic for every outlier, so its sign, and with it the
    edge's weight along its residual, is decided by the last bit of e2 (tests/golden/make_golden_huber.py, csrc/vio_device_math.h);
  - Tukey with a landmark whose every edge lies beyond delta: h_ll = 0, a non-finite step
    (test_gpu_parity.py::test_landmark_without_information_gives_an_error_not_a_crash)."""
import ctypes as C
import functools

import numpy as np

from conftest import load_package

QUIET = dict(pos_noise=0.001, rot_noise=0.0002, depth_noise=0.003, pixel_noise=0.25 / 460, outlier_fraction=0.05)
LAMBDA_GN = 5e5
GN_ITERATIONS = 3

# fields that are not named keep vio_default_config's value
CONFIGS = {
    "default": {},
    "huber_d50": dict(loss_type=1, loss_delta=50.0),
    "huber_d50_free": dict(loss_type=1, loss_delta=50.0, ext_fixed=0),
    "cauchy_d0.25": dict(loss_delta=0.25),
    "cauchy_d5_free": dict(loss_delta=5.0, ext_fixed=0),
    "trivial_s100": dict(loss_type=0, reproj_sqrt_info=100.0),
    "tukey_d1": dict(loss_type=3, loss_delta=1.0),
    "tukey_d3_free": dict(loss_type=3, loss_delta=3.0, ext_fixed=0),
    "s30": dict(reproj_sqrt_info=30.0),
    "s3000_free": dict(reproj_sqrt_info=3000.0, ext_fixed=0),
    "g_tilted": dict(gravity=(0.3, -0.2, 9.7)),
    "g_moon_free": dict(gravity=(0.0, 0.0, 1.62), ext_fixed=0),
}
TUKEY = ("tukey_d1", "tukey_d3_free")
# the XYZ landmark kind carries no extrinsic block: ext_fixed is left alone there (config_of drops it); no Tukey
XYZ_ROWS = ("huber_d50", "cauchy_d0.25", "cauchy_d5_free", "trivial_s100", "s30", "s3000_free", "g_tilted")

# (window, configuration): Tukey on the quiet window only
STEP_PAIRS = ([(w, c) for w in ("W65", "W300") for c in CONFIGS if c != "default" and c not in TUKEY] +
              [("W65Q", c) for c in TUKEY] + [("X300", c) for c in XYZ_ROWS])
# The three GN iterations of an XYZ window leave the landmarks undamped, and a ragged window has landmarks seen from two frames a tenth
# of a second apart: under the weaker weights their depth is so loosely held that one-ulp perturbations of the inputs move the oracle's
# own three-GN landmarks by 2e-11 (cauchy_d0.25), 1e-10 (s30) and 3e-7 (cauchy_d5) on X300.  Those three rows take the same window with
# another seed for the GN comparison (tests/test_config_cases_cpu.py holds each to the same 1e-11); their stepwise comparison stays on X300.
XYZ_GN_SEEDS = {"cauchy_d0.25": 43, "s30": 43, "cauchy_d5_free": 61}
GN_PAIRS = [(("X300s%d" % XYZ_GN_SEEDS[c]) if w == "X300" and c in XYZ_GN_SEEDS else w, c) for w, c in STEP_PAIRS]
# Solve(10): the pairs vetted on the oracle (same decisions and an end state that holds still under one-ulp perturbations)
SOLVE_PAIRS = [("W300", c) for c in ("huber_d50_free", "cauchy_d0.25", "cauchy_d5_free", "trivial_s100", "s30", "s3000_free", "g_tilted")] + \
              [("W65Q", "tukey_d3_free")]
SEPARATION_CASES = [("W300", c) for c in ("s30", "g_tilted", "cauchy_d5_free")]

# vio_set_config on a living context, a load after each link: the overrides accumulate
CHAIN = [
    ("loss only", dict(loss_type=1, loss_delta=50.0)),
    ("ext_fixed 1 -> 0", dict(ext_fixed=0)),
    ("information and gravity", dict(reproj_sqrt_info=100.0, gravity=(0.1, 0.0, 9.8))),
    ("item_policy 0 -> 1", dict(item_policy=1)),
    ("ext_fixed 0 -> 1", dict(ext_fixed=1)),
    ("defaults", dict(loss_type=2, loss_delta=1.0, reproj_sqrt_info=460 / 1.5, gravity=(0.0, 0.0, 9.81), item_policy=0, ext_fixed=1)),
]
# vio_set_config in the middle of a GN sequence, no load: two iterations, the change, two more
MID_GN_CHANGES = {"gravity_and_delta": dict(gravity=(0.3, -0.2, 9.7), loss_delta=5.0), "ext_fixed_1_to_0": dict(ext_fixed=0)}
# the legs of the prior test: every leg is set_config (but the first), load, three GN iterations
PRIOR_LEGS = [dict(ext_fixed=1), dict(ext_fixed=0), dict(ext_fixed=1)]
# a batch whose members differ: neighbours never share a window or a table
BATCH_MEMBERS = [("W300", "default"), ("W65", "cauchy_d0.25"), ("W300", "huber_d50_free"), ("W65", "trivial_s100"), ("W300", "s3000_free"),
                 ("W65", "g_tilted")]
# (members, change without a load), in this order and each followed by iterations of its own.  The first needs no new plan and goes to
# every member, so nothing but the members' table generations tells the leader that its device array of the tables is stale: a change
# on one member alone settles that member's owed step test, and members that differ in that make the leader build the array again anyway;
# so does the new plan that the second change needs.  BATCH_WATCHED: the member that is also compared with a twin that never changed.
BATCH_CHANGES = [((0, 1, 2, 3, 4, 5), dict(gravity=(0.0, 0.0, 1.62))), ((2,), dict(ext_fixed=1))]
BATCH_WATCHED = 1
# iterations before the members are read and compared; one more that nobody reads, so that the leader's array is current when the first
# change comes; iterations after each change
BATCH_ITERATIONS = (5, 1, 2)


@functools.lru_cache(maxsize=None)
def window(name):
    """The four windows, made once; callers load them and leave them unchanged."""
    synth = load_package().synth
    if name == "W65":          # an item tail of one landmark
        return synth.make_window(65, seed=4)
    if name == "W300":         # every (host, track-length) pattern
        return synth.make_window(300, seed=5, ragged=True)
    if name == "W65Q":
        return synth.make_window(65, seed=4, **QUIET)
    if name == "X300":
        return synth.make_window_xyz(300, seed=5, ragged=True)
    if name.startswith("X300s"):
        return synth.make_window_xyz(300, seed=int(name[5:]), ragged=True)
    raise KeyError(name)


def is_xyz(w):
    return getattr(w, "xyz", None) is not None


def config_of(wname, cname, **extra):
    cfg = dict(CONFIGS[cname])
    if wname.startswith("X"):
        cfg.pop("ext_fixed", None)
    cfg.update(extra)
    return cfg


def perturbed(w, draw):
    """w with every observation and landmark moved by one ulp, up or down by a seeded coin per entry"""
    rng = np.random.RandomState(7000 + draw)
    v = w.copy()
    for f in (("pts", "xyz") if is_xyz(w) else ("pts_i", "pts_j", "inv_depth")):
        a = getattr(w, f)
        up = rng.randint(0, 2, size=a.shape).astype(bool)
        setattr(v, f, np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)))
    return v


def with_state(w, st):
    """w with the states of state_of() in place of its own"""
    v = w.copy()
    v.poses, v.speed_bias, v.ext = st["poses"].copy(), st["sb"].copy(), st["ext"].copy()
    if is_xyz(w):
        v.xyz = st["lm"].copy()
    else:
        v.inv_depth = st["lm"].copy()
    return v


def state_of(ctx):
    p, s, e = ctx.get_window()
    return {"poses": p, "sb": s, "ext": e, "lm": ctx.get_landmarks() if ctx.lm_dim == 1 else ctx.get_landmarks_xyz(), "chi2": np.float64(ctx.chi2())}


STATE_KEYS = ("poses", "sb", "ext", "lm")


def state_diff(a, b):
    """largest absolute difference over poses, speed_bias, ext and landmarks"""
    return max(float(np.abs(a[k] - b[k]).max()) for k in STATE_KEYS)


def run_gn(ctx, iterations=GN_ITERATIONS, lam=LAMBDA_GN):
    for _ in range(iterations):
        ctx.gn_iteration(lam)
    return state_of(ctx)


def gn_state(lib, w, cfg, iterations=GN_ITERATIONS):
    ctx = lib.context(**cfg)
    ctx.load(w)
    return run_gn(ctx, iterations)


def mid_gn_sequence(ctx, change, read_back=True):
    """two GN iterations, vio_set_config(change) without a load, two more; (state just before the change or None, end state)"""
    for _ in range(2):
        ctx.gn_iteration(LAMBDA_GN)
    before = state_of(ctx) if read_back else None
    ctx.set_config(**change)
    return before, run_gn(ctx, 2)


@functools.lru_cache(maxsize=None)
def prior_of_the_oracle(oracle_path):
    """a marginalisation prior as windows() of tests/test_gpu_batch.py makes one (test infrastructure makes the input, not the result)"""
    vio = load_package()
    co = vio.VioLib(oracle_path, "vioo_").context()
    wp = vio.synth.make_window(120, seed=9)
    co.load(wp)
    co.solve(10)
    p, s, e = co.get_window()
    wp.poses, wp.speed_bias, wp.ext, wp.inv_depth = p, s, e, co.get_landmarks()
    co.load(wp)
    return co.marginalize(vio.MARG_OLD)


def window_with_prior(oracle_lib):
    w = window("W300").copy()
    w.prior = prior_of_the_oracle(oracle_lib.path)
    return w


def edge_e2(oracle_lib, w, st, sqrt_info):
    """every reprojection edge's whitened squared residual at the states st (state_of), through the oracle's edge functions as
    tests/golden/make_golden_huber.py forms it"""
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    r, out = np.zeros(2), np.zeros(w.lm.size)
    if is_xyz(w):
        f = oracle_lib.dll.vioo_reproj_xyz_edge
        f.restype = None
        for e in range(w.lm.size):
            f(dp(st["poses"][w.frame[e]]), dp(st["ext"]), dp(st["lm"][w.lm[e]]), dp(w.pts[e]), dp(r), None, None)
            out[e] = float(r @ r) * sqrt_info ** 2
        return out
    f = oracle_lib.dll.vioo_reproj_edge
    f.restype = None
    for e in range(w.lm.size):
        f(dp(st["poses"][w.host[e]]), dp(st["poses"][w.target[e]]), dp(st["ext"]), C.c_double(st["lm"][w.lm[e]]), dp(w.pts_i[e]), dp(w.pts_j[e]),
          dp(r), None, None, None, None)
        out[e] = float(r @ r) * sqrt_info ** 2
    return out


def input_state(w):
    return {"poses": w.poses, "sb": w.speed_bias, "ext": w.ext, "lm": w.xyz if is_xyz(w) else w.inv_depth}


# ---- the oracle's side of every comparison, computed once per session and left unchanged ---------------------------------------
_ORACLE = {}


def oracle_run(oracle_lib, kind, wname, cname, compute):
    key = (kind, wname, cname)
    if key not in _ORACLE:
        _ORACLE[key] = compute()
    return _ORACLE[key]


def oracle_stepwise(oracle_lib, wname, cname):
    import vio_testutil as tu

    def compute():
        c = oracle_lib.context(**config_of(wname, cname))
        c.load(window(wname))
        return tu.run_stepwise(c)
    return oracle_run(oracle_lib, "step", wname, cname, compute)


def oracle_gn(oracle_lib, wname, cname):
    return oracle_run(oracle_lib, "gn", wname, cname, lambda: gn_state(oracle_lib, window(wname), config_of(wname, cname)))


def oracle_solve(oracle_lib, wname, cname):
    import vio_testutil as tu

    def compute():
        c = oracle_lib.context(**config_of(wname, cname))
        c.load(window(wname))
        return tu.run_solve(c, 10)
    return oracle_run(oracle_lib, "solve", wname, cname, compute)
