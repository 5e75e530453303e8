"""The numpy restatement of the batched marginalisation (tests/marg_reference.py) against the oracle, on the inverse-depth golden windows
(both kinds) and the reference's marginalisation KAT.

  build: H_marg / b_marg against the oracle's own dense input (vioo_marg_dense_input) to rounding.
  tail:  test_oracle_golden.check_prior's invariants against the oracle's prior (spectrum, damped energy, err = -Jt_inv b, H P H = H), and
         the two entry-wise bars (H: 2e-5, b: 1e-6) against the Schur complement evaluated in 50-digit arithmetic from the same fp64 input,
         which is what both fp64 tails approximate.  The oracle's own QL tail misses that value by up to 8e-5 (H) and 2e-5 (b) on the
         windows with an IMU edge (Amm's condition number is ~1e11), so the oracle's prior is not the yardstick for those two entries."""
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
