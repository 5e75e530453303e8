"""What tests/test_gpu_config.py assumes of its cases, asserted on the oracle alone (no GPU): every (window, configuration) pair
is well-conditioned — moving every observation and landmark by one ulp moves the oracle's own step and its three-GN state by at most
1e-11, three decades below the 1e-8 the device is held to —, differs from the default configuration, keeps every Huber edge an inlier
and every Tukey landmark informed; Solve(10) takes the same decisions under the perturbations; and the oracle's own vio_set_config
on a living context equals a fresh context bit for bit, which licenses it as the yardstick of the device's.

The 1e-11 is a condition on the case, not a tolerance of the code: a case that breaks it is replaced, the bound stays.
Measured (printed by the tests, -s): see DESIGN.md section 40."""
import numpy as np
import pytest

import config_cases as cc
import vio_testutil as tu

DRAWS = (0, 1)
COND = 1e-11          # one-ulp perturbations of the inputs: the oracle's own answers hold still to this
BITES = 1e-4


def ids(pairs):
    return ["%s-%s" % p for p in pairs]


def stepwise(lib, w, cfg):
    c = lib.context(**cfg)
    c.load(w)
    return tu.run_stepwise(c)


ALL_PAIRS = cc.STEP_PAIRS + [p for p in cc.GN_PAIRS if p not in cc.STEP_PAIRS]


@pytest.mark.parametrize("wname,cname", ALL_PAIRS, ids=ids(ALL_PAIRS))
def test_case_is_well_conditioned_and_bites(oracle_lib, wname, cname):
    w, cfg = cc.window(wname), cc.config_of(wname, cname)
    step, gn = cc.oracle_stepwise(oracle_lib, wname, cname), cc.oracle_gn(oracle_lib, wname, cname)
    d_step = d_gn = d_chi = 0.0
    for draw in DRAWS:
        v = cc.perturbed(w, draw)
        sv = stepwise(oracle_lib, v, cfg)
        d_step = max(d_step, float(np.abs(sv["dx_pose"] - step["dx_pose"]).max()), float(np.abs(sv["dx_lm"] - step["dx_lm"]).max()))
        gv = cc.gn_state(oracle_lib, v, cfg)
        d_gn = max(d_gn, cc.state_diff(gv, gn))
        d_chi = max(d_chi, abs(gv["chi2"] - gn["chi2"]) / abs(gn["chi2"]))
    bite = cc.state_diff(gn, cc.oracle_gn(oracle_lib, wname, "default"))
    print("\n%s %s: spread under one-ulp perturbations: dx %.1e, three-GN state %.1e, chi2 %.1e (relative); differs from the default by %.1e"
          % (wname, cname, d_step, d_gn, d_chi, bite))
    in_step, in_gn = (wname, cname) in cc.STEP_PAIRS, (wname, cname) in cc.GN_PAIRS
    assert d_step <= COND or not in_step
    assert (d_gn <= COND and d_chi <= COND and bite >= BITES) or not in_gn
    if cfg.get("loss_type") == 1:
        # Huber: every edge an inlier at the linearisation point and after each of the three iterations
        s_info = cfg.get("reproj_sqrt_info", oracle_lib.default_config().reproj_sqrt_info)
        c = oracle_lib.context(**cfg)
        c.load(w)
        e2 = [cc.edge_e2(oracle_lib, w, cc.input_state(w), s_info).max()]
        for _ in range(cc.GN_ITERATIONS):
            c.gn_iteration(cc.LAMBDA_GN)
            e2.append(cc.edge_e2(oracle_lib, w, cc.state_of(c), s_info).max())
        print("  Huber: largest e2 at the linearisation point and after each iteration:", ["%.1f" % v for v in e2], "delta^2 = %g" % cfg["loss_delta"] ** 2)
        assert max(e2) < cfg["loss_delta"] ** 2
        assert cc.edge_e2(oracle_lib, w, {"poses": step["poses1"], "sb": step["sb1"], "ext": step["ext1"], "lm": step["invd1"]}, s_info).max() < cfg["loss_delta"] ** 2
    if cfg.get("loss_type") == 3:
        # Tukey: every landmark keeps information
        assert all(np.isfinite(step[k]).all() for k in ("dx_pose", "dx_lm", "Hs", "bs", "poses1", "invd1")) and np.isfinite(step["chi1"])
        assert int(step["accepted"]) == 1 and step["hll"].min() > 0


@pytest.mark.parametrize("wname,cname", cc.SOLVE_PAIRS, ids=ids(cc.SOLVE_PAIRS))
def test_solve_takes_the_same_decisions_under_perturbations(oracle_lib, wname, cname):
    w, cfg = cc.window(wname), cc.config_of(wname, cname)
    sol, rep = cc.oracle_solve(oracle_lib, wname, cname)
    what = (rep.iterations, rep.trials, rep.accepted, rep.stop_reason)
    spread = 0.0
    for draw in DRAWS:
        c = oracle_lib.context(**cfg)
        c.load(cc.perturbed(w, draw))
        sv, rv = tu.run_solve(c, 10)
        assert (rv.iterations, rv.trials, rv.accepted, rv.stop_reason) == what
        spread = max(spread, max(float(np.abs(sv[k] - sol[k]).max()) for k in ("posesF", "sbF", "extF", "invdF")))
    print("\n%s %s: Solve(10) iterations/trials/accepted/stop %s, end-state spread %.1e" % (wname, cname, what, spread))
    assert spread <= 1e-10
    if cfg.get("loss_type") == 1:
        s_info = cfg.get("reproj_sqrt_info", oracle_lib.default_config().reproj_sqrt_info)
        e2 = cc.edge_e2(oracle_lib, w, {"poses": sol["posesF"], "sb": sol["sbF"], "ext": sol["extF"], "lm": sol["invdF"]}, s_info).max()
        assert e2 < cfg["loss_delta"] ** 2


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_oracle_set_config_with_a_load_equals_a_fresh_context(oracle_lib):
    w = cc.window("W300")
    live = oracle_lib.context()
    live.load(w)
    first = tu.run_stepwise(live)
    acc = {}
    for name, change in cc.CHAIN:
        acc.update(change)
        live.set_config(**change)
        live.load(w)
        got = tu.run_stepwise(live)
        assert_same_bits(got, stepwise(oracle_lib, w, acc))
    assert_same_bits(got, first)


@pytest.mark.parametrize("change", list(cc.MID_GN_CHANGES))
def test_oracle_set_config_in_the_middle_of_a_gn_sequence(oracle_lib, change):
    w, kw = cc.window("W300"), cc.MID_GN_CHANGES[change]
    live = oracle_lib.context()
    live.load(w)
    before, end = cc.mid_gn_sequence(live, kw)
    fresh = oracle_lib.context(**kw)
    fresh.load(cc.with_state(w, before))
    assert_same_bits(cc.run_gn(fresh, 2), end)
    # the sequence is as well-conditioned as the single cases, and the change bites
    spread = 0.0
    for draw in DRAWS:
        c = oracle_lib.context()
        c.load(cc.perturbed(w, draw))
        _, ev = cc.mid_gn_sequence(c, kw)
        spread = max(spread, cc.state_diff(ev, end), abs(ev["chi2"] - end["chi2"]) / abs(end["chi2"]))
    bite = cc.state_diff(end, cc.gn_state(oracle_lib, w, {}, 4))
    print("\nW300, set_config(%s) after two of four GN iterations: spread %.1e, differs from four unchanged iterations by %.1e" % (change, spread, bite))
    assert spread <= COND and bite >= BITES


def test_prior_legs_are_well_conditioned(oracle_lib):
    w = cc.window_with_prior(oracle_lib)
    ends = []
    for leg in cc.PRIOR_LEGS:
        end = cc.gn_state(oracle_lib, w, leg)
        spread = 0.0
        for draw in DRAWS:
            ev = cc.gn_state(oracle_lib, cc.perturbed(w, draw), leg)
            spread = max(spread, cc.state_diff(ev, end), abs(ev["chi2"] - end["chi2"]) / abs(end["chi2"]))
        print("\nW300 with a prior, %s: three-GN spread %.1e" % (leg, spread))
        assert spread <= COND
        ends.append(end)
    assert cc.state_diff(ends[0], ends[1]) >= BITES        # the free extrinsic moves
    assert cc.state_diff(ends[0], cc.oracle_gn(oracle_lib, "W300", "default")) >= BITES        # and the prior is felt


def test_batch_change_bites(oracle_lib):
    """the first change of the batch test: gravity changed after six GN iterations; two more differ from two unchanged ones"""
    _, change = cc.BATCH_CHANGES[0]
    wname, cname = cc.BATCH_MEMBERS[cc.BATCH_WATCHED]
    w, cfg = cc.window(wname), cc.config_of(wname, cname)
    n0, n1 = sum(cc.BATCH_ITERATIONS[:2]), cc.BATCH_ITERATIONS[2]
    c = oracle_lib.context(**cfg)
    c.load(w)
    cc.run_gn(c, n0)
    c.set_config(**change)
    bite = cc.state_diff(cc.run_gn(c, n1), cc.gn_state(oracle_lib, w, cfg, n0 + n1))
    print("\n%s %s: gravity changed after %d iterations, %d more differ from unchanged ones by %.1e" % (wname, cname, n0, n1, bite))
    assert bite >= BITES
