"""The numpy restatement of the batched marginalisation (tests/marg_reference.py) against the oracle, on the inverse-depth golden windows
(both kinds) and the reference's marginalisation KAT.

  build: H_marg / b_marg against the oracle's own dense input (vioo_marg_dense_input) to rounding.
  tail:  test_oracle_golden.check_prior's invariants against the oracle's prior (spectrum, damped energy, err = -Jt_inv b, H P H = H), and
         the two entry-wise bars (H: 2e-5, b: 1e-6) against the Schur complement evaluated in 50-digit arithmetic from the same fp64 input,
         which is what both fp64 tails approximate.  The oracle's own QL tail misses that value by up to 8e-5 (H) and 2e-5 (b) on the
         windows with an IMU edge (Amm's condition number is ~1e11), so the oracle's prior is not the yardstick for those two entries.
  limits: the well-conditioned windows of test_gpu_marg_limits.py (marg_reference.limit_cases): the restatement and the oracle each within
         1e-12 of the exact Schur complement (tight_check with the other as the only reference), the spectrum invariants, the two
         nothing-live systems, Tukey 3's landmark without an inverse, and the packer's rules on build."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marg_reference as mr  # noqa: E402
import vio_testutil as tu  # noqa: E402
from test_oracle_golden import cfg_of, check_prior  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOWS = ["window_n50_s42", "window_n300_s43", "window_n300_s45_prior", "window_n200_s46_huber", "window_n200_s46_tukey",
           "window_n120_s44_ragged_extfree", "window_noimu_n300_s48_prior"]


def check_against_exact(m, ref, Hin, bin_, frame):
    """check_prior, with its two entry-wise comparisons made against the exact Schur complement of the common input: m must be within
    check_prior's bars of it (H 2e-5, b 1e-6), or no farther from it than the oracle's own prior is."""
    live = np.nonzero(np.abs(ref["H"]).sum(1) > 0)[0]
    S, bs = mr.exact_schur(Hin, bin_, frame, live)
    Ss, bsc = np.abs(S).max(), max(np.abs(bs).max(), 1.0)
    lv = np.ix_(live, live)
    assert np.abs(m["H"][lv] - S).max() <= max(2e-5 * Ss, np.abs(ref["H"][lv] - S).max())
    assert np.abs(m["b"][live] - bs).max() <= max(1e-6 * bsc, np.abs(ref["b"][live] - bs).max())
    # err = -Jt_inv b, evaluated in extended precision (the dot products cancel by orders of magnitude on large windows)
    r = m["err"].astype(np.longdouble) + m["jt_inv"].astype(np.longdouble) @ m["b"].astype(np.longdouble)
    assert float(np.abs(r).max()) <= 1e-9 * max(np.abs(m["err"]).max(), 1e-12)
    m2 = dict(m, err=-(m["jt_inv"] @ m["b"]))              # (check_prior's own consistency test is the fp64 one just made exactly)
    check_prior(m2, dict(ref, H=m["H"], b=m["b"]))       # (every other invariant, against the oracle's prior where it compares)
    ev, evr = np.linalg.eigvalsh(m["H"]), np.linalg.eigvalsh(ref["H"])
    assert np.abs(ev - evr).max() <= 2e-5 * evr.max()
    mu = 1e-4 * np.linalg.eigvalsh(0.5 * (ref["H"] + ref["H"].T)).max()

    def energy(H, b):
        return float(b @ np.linalg.solve(0.5 * (H + H.T) + mu * np.eye(H.shape[0]), b))
    assert abs(energy(m["H"], m["b"]) - energy(ref["H"], ref["b"])) <= 5e-3 * max(energy(ref["H"], ref["b"]), 1e-9)


@pytest.mark.parametrize("kind", [0, 1], ids=["old", "second_new"])
@pytest.mark.parametrize("name", WINDOWS)
def test_restatement_against_the_oracle(vio, oracle_lib, name, kind):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    w, kw = tu.arrays_to_window(vio, z), cfg_of(z)
    if kind == vio.MARG_SECOND_NEW and w.prior is None:
        c0 = oracle_lib.context(**kw)
        c0.load(w)
        w.prior = c0.marginalize(vio.MARG_OLD)
    c = oracle_lib.context(**kw)
    c.load(w)
    Hd, bd = mr.dense_input(oracle_lib, c, kind)
    H, b = mr.build(oracle_lib, vio, c.cfg, kind, w, w.prior)
    assert np.abs(H - Hd).max() <= 1e-14 * np.abs(Hd).max()
    assert np.abs(b - bd).max() <= 1e-14 * max(np.abs(bd).max(), 1.0)
    ref = c.marginalize(kind)
    m, live = mr.tail(H, b, 0 if kind == vio.MARG_OLD else vio.WINDOW_SIZE - 1)
    assert live == int((np.abs(ref["H"]).sum(1) > 0).sum())
    check_against_exact(m, ref, H, b, 0 if kind == vio.MARG_OLD else vio.WINDOW_SIZE - 1)


def test_restatement_reproduces_the_marg_kat(vio):
    import test_marg_kat as kat
    p = kat.kat_prior()
    H, b = np.zeros((171, 171)), np.zeros(171)
    H[:156, :156] = p["H"]
    m, live = mr.tail(H, b, vio.WINDOW_SIZE - 1)
    kat.check_output(m)


def test_jacobi_solver_on_its_own():
    rng = np.random.RandomState(4)
    for n in (2, 16, 40, 76, 156):
        A = rng.normal(size=(n, n))
        A = A @ A.T + np.diag(np.geomspace(1e-6, 1e6, n))
        ev, Vt = mr.jacobi(A)
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-12 * np.abs(ev).max()
        assert np.abs(Vt @ Vt.T - np.eye(n)).max() <= 1e-13
        assert np.abs((Vt.T * ev) @ Vt - A).max() <= 1e-12 * np.abs(A).max()


# ---------------------------------------------------------------------------------------------------------
# the well-conditioned windows of test_gpu_marg_limits.py: the references themselves, on the CPU
# ---------------------------------------------------------------------------------------------------------
def check_references(oracle_lib, name, kind, w, kw, spectrum_expected):
    """The restatement and the oracle each within tight_check of the exact Schur complement with the other as the only reference and
    an absolute ceiling of 1e-12 (measured: 3.3e-14 at most for H, 4.5e-14 for b): this is not the device's bar, it keeps the references
    from drifting.  The spectrum invariants on both; the band around the 1e-8 cut is empty exactly where SPECTRUM_CASES says."""
    Hin, bin_, rest, orc = mr.references(oracle_lib, kind, w, kw)
    frame = mr.frame_of(kind)
    mr.tight_check(rest, Hin, bin_, frame, [orc], ceiling=1e-12, name=name + " restatement")
    mr.tight_check(orc, Hin, bin_, frame, [rest], ceiling=1e-12, name=name + " oracle", dead_rows_exact=False)
    ev = mr.tail_full(Hin, bin_, frame)[3]
    assert mr.band_is_empty(ev) == spectrum_expected, (name, np.sort(np.abs(ev))[:4])
    assert mr.spectrum_check(rest, Hin, bin_, frame, orc, name) == spectrum_expected
    assert mr.spectrum_check(orc, Hin, bin_, frame, orc, name) == spectrum_expected
    return Hin, bin_, rest, orc


@pytest.mark.parametrize("name", mr.LIMIT_NAMES)
def test_limit_window_references(vio, oracle_lib, name):
    kind, w, kw, amb = mr.limit_case(name)
    if amb:
        w = mr.drop_huber_ambiguous(oracle_lib, w, kw)
    Hin, bin_, rest, orc = check_references(oracle_lib, name, kind, w, kw, name in mr.SPECTRUM_CASES)
    if name in mr.EXPECT_LIVE:
        assert len(mr.live_set(rest["H"])) == mr.EXPECT_LIVE[name]
    if w.n_landmarks <= 60:            # (build's Python loop is slow beyond; dense_input is what the GPU tests feed the tail)
        c = oracle_lib.context(**kw)
        H, b = mr.build(oracle_lib, vio, c.cfg, kind, w, w.prior)
        assert np.abs(H - Hin).max() <= 1e-14 * max(np.abs(Hin).max(), 1.0)
        assert np.abs(b - bin_).max() <= 1e-14 * max(np.abs(bin_).max(), 1.0)


def test_limit_window_list_is_the_one_made():
    assert list(mr.limit_cases()) == mr.LIMIT_NAMES and set(mr.SPECTRUM_CASES) <= set(mr.LIMIT_NAMES) and len(mr.SPECTRUM_CASES) - 1 >= 6
    assert mr.limit_case("noimu_huber10_halfinfo")[1].n_landmarks == 40


def test_second_stage_references(vio, oracle_lib):
    """ragged300's prior (here the restatement's) fed back as the prior of the second stage."""
    kind, w, kw, _ = mr.limit_case("ragged300")
    rest = mr.references(oracle_lib, kind, w, kw)[2]
    w2 = mr.second_stage(rest)
    Hin, bin_, r2, o2 = mr.references(oracle_lib, vio.MARG_OLD, w2, {})
    ev = mr.tail_full(Hin, bin_, 0)[3]
    check_references(oracle_lib, "second stage", vio.MARG_OLD, w2, {}, mr.band_is_empty(ev))
    assert len(mr.live_set(r2["H"])) == 75 and np.abs(w2.prior["H"]).max() > 0


def test_gravity_reaches_b(vio, oracle_lib):
    """The non-default gravity moves b by far more than tight_check's bar (1e-13 of max(|b|, 1))."""
    k, w, kw, _ = mr.limit_case("soft_1e-4")
    k2, w2, kw2, _ = mr.limit_case("soft_1e-4_gravity")
    a, b = mr.references(oracle_lib, k, w, kw)[2], mr.references(oracle_lib, k2, w2, kw2)[2]
    assert np.abs(a["b"] - b["b"]).max() >= 1e-3 * max(np.abs(a["b"]).max(), 1.0)


@pytest.mark.parametrize("case", ["marg_old", "second_new"])
def test_nothing_live(vio, oracle_lib, case):
    """MARG_OLD without prior, IMU edge 0 or frame-0 hosts, and MARG_SECOND_NEW of a prior inside frame 9's block: H = jt_inv = 0,
    err = b = 0, no live row, from the restatement and from the oracle."""
    if case == "marg_old":
        kind, w = vio.MARG_OLD, mr.nothing_live_window()
    else:
        kind, w = vio.MARG_SECOND_NEW, vio.synth.make_window(8, seed=3)
        w.prior = mr.frame9_only_prior()
    Hin, bin_, rest, orc = mr.references(oracle_lib, kind, w, {})
    assert mr.tail(Hin, bin_, mr.frame_of(kind))[1] == 0
    for m in (rest, orc):
        assert all(not m[k].any() for k in ("H", "b", "err", "jt_inv"))


def test_tukey_3_leaves_a_landmark_without_an_inverse(vio, oracle_lib):
    """Every edge of one frame-0 landmark of the outlier window lies beyond Tukey's delta = 3: h = 0 exactly, the non-finite outcome
    (H 0, the rest NaN) from both, and the oracle's status says so."""
    w, kw = mr.tukey3_window()
    c = oracle_lib.context(**kw)
    c.load(w)
    with pytest.raises(vio.VioError) as ei:
        c.marginalize(vio.MARG_OLD)
    assert ei.value.status == -3
    Hin, bin_, rest, orc = mr.references(oracle_lib, vio.MARG_OLD, w, kw)
    assert not np.isfinite(Hin).all()
    for m in (rest, orc):
        assert not m["H"].any() and all(np.isnan(m[k]).all() for k in ("b", "err", "jt_inv"))
    # the neighbours the GPU test puts beside it are ordinary under that loss
    for seed in (1, 2, 3):
        assert np.isfinite(mr.references(oracle_lib, vio.MARG_OLD, mr.quiet_window(30, seed), kw)[0]).all()


def test_build_follows_the_packers_rules(vio, oracle_lib):
    """mr.build gives the same bits whatever the order in which landmarks interleave, with or without the landmarks outside
    MargOldFrame's graph (other hosts, no observation), and whatever an edge outside the graph holds."""
    w = mr.packer_window()
    assert (np.asarray(w.host) == 0).sum() > 0 and (np.asarray(w.host) == 3).sum() > 1
    cfg = oracle_lib.context().cfg
    H0, b0 = mr.build(oracle_lib, vio, cfg, vio.MARG_OLD, w, None)
    for name, v in (("interleaved", mr.interleaved(w)), ("only_frame0", mr.only_frame0(w)),
                    ("unobserved", mr.with_unobserved_landmark(w)), ("nan_outside", mr.nan_outside_graph(w))):
        assert not np.array_equal(np.asarray(v.lm), np.asarray(w.lm)) or name in ("unobserved", "nan_outside")
        H, b = mr.build(oracle_lib, vio, cfg, vio.MARG_OLD, v, None)
        assert np.array_equal(H, H0) and np.array_equal(b, b0), name
