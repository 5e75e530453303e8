"""The window solver off vio_default_config and across vio_set_config: the loss, its delta, the reprojection
information and gravity reach the kernels as fields of DeviceTables that several independent sites read, in every instantiation
(full and half-width workgroups, extrinsic block or not, inverse depth or XYZ, solo or batched); the host keeps state of its own
across vio_set_config.  A literal left behind at one site, a site that reads the batch leader's table, a table that survives a
vio_set_config: each shows here as a difference to the oracle or to a fresh context.

The cases are tests/config_cases.py's; tests/test_config_cases_cpu.py asserts on the oracle alone that each is well-conditioned
(one-ulp perturbations of the inputs move the oracle's own answer by at most 1e-11), differs from the default, keeps Huber's edges
inliers and Tukey's landmarks informed.  No tolerance is chosen here: compare_stepwise is test_gpu_parity.py's (XYZ:
test_xyz_landmarks.py's), GN sequences take the rule of test_gn_iterations_interleaved_with_everything_else (XYZ:
test_hip_gn_iterations_against_oracle), Solve(10) the rule of test_full_solve_against_oracle, "the same bits" is assert_array_equal."""
import numpy as np
import pytest

import config_cases as cc
import vio_testutil as tu
from test_gpu_parity import compare_stepwise
from test_xyz_landmarks import compare_stepwise as compare_stepwise_xyz

pytestmark = pytest.mark.gpu
POLICIES = (0, 1)          # VIO_ITEMS_LATENCY; VIO_ITEMS_THROUGHPUT: the half-width kernels, bodies of their own


def ids(pairs):
    return ["%s-%s" % p for p in pairs]


def gn_rule(a, b, xyz=False):
    """a: device, b: oracle (config_cases.state_of)"""
    if xyz:          # test_xyz_landmarks.py::test_hip_gn_iterations_against_oracle
        assert np.abs(a["poses"] - b["poses"]).max() <= 1e-6 and np.abs(a["sb"] - b["sb"]).max() <= 1e-6 and np.abs(a["ext"] - b["ext"]).max() <= 1e-6
        assert np.abs(a["lm"] - b["lm"]).max() <= 3e-6
        assert abs(a["chi2"] - b["chi2"]) <= 1e-7 * b["chi2"]
        return
    assert abs(a["chi2"] - b["chi2"]) <= 1e-9 * b["chi2"]
    np.testing.assert_allclose(a["lm"], b["lm"], rtol=1e-8, atol=1e-10)
    for k in ("poses", "sb", "ext"):
        assert np.abs(a[k] - b[k]).max() <= 1e-8, k


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def stepwise(lib, w, cfg):
    c = lib.context(**cfg)
    c.load(w)
    return tu.run_stepwise(c)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("wname,cname", cc.STEP_PAIRS, ids=ids(cc.STEP_PAIRS))
def test_every_case_stepwise_against_the_oracle(oracle_lib, hip_lib, wname, cname, policy):
    w = cc.window(wname)
    a = stepwise(hip_lib, w, cc.config_of(wname, cname, item_policy=policy))
    b = cc.oracle_stepwise(oracle_lib, wname, cname)
    print("\n%s %s policy %d: largest |dx - oracle's| %.1e" % (wname, cname, policy, max(np.abs(a["dx_pose"] - b["dx_pose"]).max(), np.abs(a["dx_lm"] - b["dx_lm"]).max())))
    (compare_stepwise_xyz if cc.is_xyz(w) else compare_stepwise)(a, b)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("wname,cname", cc.GN_PAIRS, ids=ids(cc.GN_PAIRS))
def test_every_case_through_the_gn_path(oracle_lib, hip_lib, wname, cname, policy):
    w = cc.window(wname)
    a = cc.gn_state(hip_lib, w, cc.config_of(wname, cname, item_policy=policy))
    b = cc.oracle_gn(oracle_lib, wname, cname)
    print("\n%s %s policy %d: largest |state - oracle's| after three GN iterations %.1e, chi2 %.1e (relative)"
          % (wname, cname, policy, cc.state_diff(a, b), abs(a["chi2"] - b["chi2"]) / b["chi2"]))
    gn_rule(a, b, cc.is_xyz(w))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("wname,cname", cc.SOLVE_PAIRS, ids=ids(cc.SOLVE_PAIRS))
def test_every_case_through_vio_solve(oracle_lib, hip_lib, wname, cname, policy):
    ch = hip_lib.context(**cc.config_of(wname, cname, item_policy=policy))
    ch.load(cc.window(wname))
    sh, rh = tu.run_solve(ch, 10)
    so, ro = cc.oracle_solve(oracle_lib, wname, cname)
    print("\n%s %s policy %d: Solve(10) largest |end state - oracle's| %.1e" % (wname, cname, policy, max(np.abs(sh[k] - so[k]).max() for k in ("posesF", "sbF", "extF", "invdF"))))
    assert (rh.iterations, rh.trials, rh.accepted, rh.stop_reason) == (ro.iterations, ro.trials, ro.accepted, ro.stop_reason)
    for k in ("posesF", "sbF", "extF", "invdF"):
        assert np.abs(sh[k] - so[k]).max() <= 1e-6, k
    assert abs(rh.final_chi2 - ro.final_chi2) <= 1e-6 * ro.final_chi2


def refused(vio, ctx, **bad):
    """vio_set_config(bad) is refused with VIO_ERR_BAD_ARG; the binding's own copy of the configuration is put back"""
    keep = {k: getattr(ctx.cfg, k) for k in bad}
    with pytest.raises(vio.VioError) as e:
        ctx.set_config(**bad)
    assert e.value.status == -1
    for k, v in keep.items():
        setattr(ctx.cfg, k, v)


def test_set_config_on_a_living_context_with_a_load_after_each_change(vio, oracle_lib, hip_lib):
    """One context through a chain of changes: loss only (no replan), ext_fixed (replan), information and gravity, item_policy
    (replan, other kernels), ext_fixed back, every field back.  After each: the bits of a fresh context of the accumulated
    configuration, and the oracle's step."""
    w = cc.window("W300")
    live = hip_lib.context()
    live.load(w)
    first = tu.run_stepwise(live)
    same_bits(first, stepwise(hip_lib, w, {}))
    acc = {}
    for name, change in cc.CHAIN:
        acc.update(change)
        live.set_config(**change)
        live.load(w)
        got = tu.run_stepwise(live)
        fresh = stepwise(hip_lib, w, acc)
        same_bits(got, fresh)
        compare_stepwise(got, stepwise(oracle_lib, w, {k: v for k, v in acc.items() if k != "item_policy"}))
        if name == "information and gravity":
            # device and shard fields belong to the context's creation: refused, and nothing of the call is taken over
            refused(vio, live, device=live.cfg.device + 1, loss_delta=7.0)
            refused(vio, live, shard_rank=1, reproj_sqrt_info=55.0)
            refused(vio, live, shard_count=2, loss_type=0)
            live.load(w)
            same_bits(tu.run_stepwise(live), fresh)
    same_bits(got, first)


@pytest.mark.parametrize("change", list(cc.MID_GN_CHANGES))
def test_set_config_in_the_middle_of_a_gn_sequence(oracle_lib, hip_lib, change):
    """Two GN iterations, vio_set_config without a load, two more: the second one's landmark update is still owed when the change
    comes (vio_set_config pulls the state, which settles it), and the states stay.  Gravity and the loss delta: the same plan;
    ext_fixed 1 -> 0: another plan, the state kept."""
    w, kw = cc.window("W300"), cc.MID_GN_CHANGES[change]
    a, b, o = hip_lib.context(), hip_lib.context(), oracle_lib.context()
    for c in (a, b, o):
        c.load(w)
    before, end = cc.mid_gn_sequence(a, kw)
    _, end_b = cc.mid_gn_sequence(b, kw, read_back=False)          # nobody looked before the change
    _, end_o = cc.mid_gn_sequence(o, kw)
    same_bits(end_b, end)
    print("\nW300 set_config(%s) after two of four GN iterations: largest |state - oracle's| %.1e" % (change, cc.state_diff(end, end_o)))
    gn_rule(end, end_o)
    fresh = hip_lib.context(**kw)
    fresh.load(cc.with_state(w, before))
    same_bits(cc.run_gn(fresh, 2), end)


def test_a_prior_across_ext_fixed(oracle_lib, hip_lib):
    """ext_fixed decides which entries of the prior are masked: vio_set_config drops the image made of it (prior_simg_valid), and
    every leg equals a fresh context of that configuration with the same prior."""
    w = cc.window_with_prior(oracle_lib)

    def with_prior(c):
        st = cc.state_of(c)
        st["bprior"], st["errprior"] = c.get_prior()
        return st

    live = hip_lib.context()
    for i, leg in enumerate(cc.PRIOR_LEGS):
        if i:
            live.set_config(**leg)
        live.load(w)
        cc.run_gn(live)
        got = with_prior(live)
        fresh, o = hip_lib.context(**leg), oracle_lib.context(**leg)
        for c in (fresh, o):
            c.load(w)
            cc.run_gn(c)
        same_bits(got, with_prior(fresh))
        ref = with_prior(o)
        print("\nW300 with a prior, leg %d %s: largest |state - oracle's| %.1e" % (i, leg, cc.state_diff(got, ref)))
        gn_rule(got, ref)
        # (test_gpu_parity.py::test_gn_iterations_with_a_prior)
        assert tu.rel_max(got["bprior"], ref["bprior"]) <= 1e-9 and tu.rel_max(got["errprior"], ref["errprior"]) <= 1e-7


@pytest.mark.parametrize("policy", POLICIES)
def test_a_batch_whose_members_differ(hip_lib, policy):
    """Six windows on one stream, each with a configuration of its own, so that a neighbour's table (or the leader's) is never
    the right one: every member equals its solo context bit for bit (the solo contexts are held to the oracle above), also
    after vio_set_config without a load — the leader must rebuild its array of the members' tables.  The change that needs no new
    plan comes first and goes to every member: then only the generation count that vio_set_config's dirty_inputs leads to tells the
    leader of it (on one member alone it settles that member's owed step test, and members that differ in that have the array
    rebuilt anyway; so has the new plan of the second change, ext_fixed on one member)."""
    members = [(cc.window(wn), cc.config_of(wn, cn, item_policy=policy)) for wn, cn in cc.BATCH_MEMBERS]

    def make():
        lead = hip_lib.context(**members[0][1])
        batch = [lead] + [hip_lib.context(stream=lead.get_stream(), **cfg) for _, cfg in members[1:]]
        solo = [hip_lib.context(**cfg) for _, cfg in members]
        for (w, _), c, r in zip(members, batch, solo):
            c.load(w)
            r.load(w)
        return batch, solo

    def check(batch, solo):
        for c, r in zip(batch, solo):
            same_bits(cc.state_of(c), cc.state_of(r))

    batch, solo = make()
    n0, n_quiet, n1 = cc.BATCH_ITERATIONS
    watched = cc.BATCH_WATCHED
    unchanged = hip_lib.context(**members[watched][1])
    unchanged.load(members[watched][0])

    def iterate(n):
        for _ in range(n):
            hip_lib.batch_gn_iteration(batch, cc.LAMBDA_GN)
            for r in solo + [unchanged]:
                r.gn_iteration(cc.LAMBDA_GN)

    iterate(n0)
    check(batch, solo)
    iterate(n_quiet)          # nobody looks between this call and the change: the leader's array of the tables is current when it comes
    for k, (who, change) in enumerate(cc.BATCH_CHANGES):
        for i in who:
            batch[i].set_config(**change)
            solo[i].set_config(**change)
        iterate(n1)
        check(batch, solo)
        if k == 0:
            assert cc.state_diff(cc.state_of(batch[watched]), cc.state_of(unchanged)) > 1e-4          # the change reached the batch's tables
    # Problem::Solve of the same six in one call (the rule of test_gpu_batch.py::test_batched_lm_solve_equals_separate_solves)
    batch, solo = make()
    for rb, c, r in zip(hip_lib.batch_solve(batch, 5), batch, solo):
        rs = r.solve(5)
        assert (rb.iterations, rb.trials, rb.accepted, rb.stop_reason) == (rs.iterations, rs.trials, rs.accepted, rs.stop_reason)
        assert rb.final_chi2 == rs.final_chi2 and rb.final_lambda == rs.final_lambda and rb.initial_chi2 == rs.initial_chi2
        np.testing.assert_array_equal(np.array(rb.chi2_trace[:]), np.array(rs.chi2_trace[:]))
        same_bits(cc.state_of(c), cc.state_of(r))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("wname,cname", cc.SEPARATION_CASES, ids=ids(cc.SEPARATION_CASES))
def test_the_device_itself_tells_the_case_from_the_default(hip_lib, wname, cname, policy):
    """Every comparison above could be made between two runs that both ignored the field; this one could not."""
    w = cc.window(wname)
    a = cc.gn_state(hip_lib, w, cc.config_of(wname, cname, item_policy=policy))
    b = cc.gn_state(hip_lib, w, cc.config_of(wname, "default", item_policy=policy))
    assert cc.state_diff(a, b) >= 1e-4
