"""The covariance query (csrc/libvio_cov_hip.so) at the edges of its landmark tile and on the inputs it refuses.

Rule: pose_cov and the landmark variances / covariances are held to the numpy reference of tests/cov_reference.py at the HIP
context's state, to cr.tolerance(S, keep) in the scaled metric, with the symmetry, zero-row and landmark-information assertions of
test_gpu_covariance.py (cr.check_cov); a refused call leaves caller-owned outputs untouched.

Shapes, from the tiles vio_covariance.hip defines (cr.lm_tile reads LmNT<1>::v = 128 and LmNT<3>::v = 64 from the source, so a
changed tile moves the shapes): one landmark less than a workgroup, a whole workgroup, and one more, for inverse depths and for XYZ
points.  `if (l >= a.n) return;` behind the staging barrier of vio_cov_landmarks_body.inc is taken by the idle lanes of such a last
workgroup (one idle lane, none, all but one).

Landmarks the caller's list has no observation of: vio_linearize refuses a window with such a landmark (VIO_ERR_UNSUPPORTED: its
Hessian block would be singular), and the query passes that refusal on with the outputs untouched.  status[1] -- the atomicMin of
the smallest landmark whose information is not positive definite -- is therefore reached the one way the ABI leaves: the context
holds the linearisation of the whole window, and the list given to the query lacks a landmark's edges (the list is the caller's to
keep consistent, include/vio_covariance.h).  Its information is then exactly 0 (test_covariance_reference.py establishes that for
the reference), the call fails with VIO_ERR_NOT_FINITE naming the smallest such landmark, and nothing is written.  The same holds
for a landmark whose edges name two host frames: the host refuses the list (VIO_ERR_BAD_ARG) before any launch.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as cr  # noqa: E402
import res_reference as rr  # noqa: E402  (take_edges)

pytestmark = pytest.mark.gpu

NT1, NT3 = cr.lm_tile(1), cr.lm_tile(3)


def test_tile_constants():
    """The literals this module's reasoning rests on, against the source text."""
    assert (NT1, NT3) == (128, 64)
    body = open(os.path.join(os.path.dirname(cr.COV_SOURCE), "vio_cov_landmarks_body.inc")).read()
    assert "const int l = blk * NT + tid;\n    if (l >= a.n) return;" in body
    assert "atomicMin(a.bad, l)" in body


def well_posed(vio, hip_lib, w, **kw):
    """A context holding w with a prior topped up from its own H_pp_schur (cr.well_posed_prior), solved."""
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY, **kw)
    c.load(w)
    c.linearize()
    S0, _ = c.get_schur_system()
    w.prior = cr.well_posed_prior(np.diag(S0))
    c.load(w)
    c.solve(5)
    return c


SIZES = [(NT1 - 1, False), (NT1, False), (NT1 + 1, False), (NT3 - 1, True), (NT3, True), (NT3 + 1, True)]


@pytest.mark.parametrize("n,xyz", SIZES, ids=["%s%d" % ("xyz" if x else "n", n) for n, x in SIZES])
def test_landmark_counts_around_a_workgroup(vio, hip_lib, oracle_lib, n, xyz):
    make = vio.synth.make_window_xyz if xyz else vio.synth.make_window
    w = make(n, seed=17, ragged=not xyz, t0=1.1)
    c = well_posed(vio, hip_lib, w)
    P, L = c.covariance(w, gauge="fix_oldest")
    cr.check_cov(oracle_lib, c, w, P, L, xyz)
    D = L.reshape(n, 3, 3) if xyz else L.reshape(n, 1, 1)
    assert np.all(np.isfinite(L)) and np.all(np.einsum("nii->ni", D) > 0)


def sentinels(n):
    return np.full((cr.PD, cr.PD), 7.0), np.full(n, 7.0)


@pytest.mark.parametrize("gone,named", [([0], 0), ([NT1], NT1), ([5, NT1], 5)], ids=["first", "last", "two"])
def test_a_landmark_the_list_has_no_edge_of(vio, hip_lib, gone, named):
    """n = LmNT<1> + 1: landmark n - 1 is the only live lane of the second workgroup, and with landmarks 5 and n - 1 both bare the
    two workgroups race to the atomicMin, which must keep the smaller."""
    n = NT1 + 1
    w = vio.synth.make_window(n, seed=18)
    c = well_posed(vio, hip_lib, w)
    P0, L0 = c.covariance(w)                                      # the whole list: fine
    assert np.all(L0 > 0)
    bare = rr.take_edges(w, ~np.isin(w.lm, gone))
    P, L = sentinels(n)
    with pytest.raises(vio.VioError) as ei:
        c._cov.compute(bare, "fix_oldest", pose_cov=P, lm_out=L)
    assert ei.value.status == -3, str(ei.value)
    assert "landmark %d: its information is not positive definite and finite" % named in str(ei.value), str(ei.value)
    assert np.all(P == 7.0) and np.all(L == 7.0)
    P1, L1 = c.covariance(w)                                      # the handle is as good as before
    assert np.array_equal(P1, P0) and np.array_equal(L1, L0)
    # a context that holds the bare window itself: the solver refuses it, the query passes that on and writes nothing
    cb = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    cb.load(bare)
    with pytest.raises(vio.VioError) as ei:
        cb.covariance(bare)                                        # (creates the handle)
    assert ei.value.status == -5 and "without observations" in str(ei.value), str(ei.value)
    with pytest.raises(vio.VioError) as ei:
        cb._cov.compute(bare, "fix_oldest", pose_cov=P, lm_out=L)
    assert ei.value.status == -5 and np.all(P == 7.0) and np.all(L == 7.0)


def test_two_host_frames_for_one_landmark(vio, hip_lib):
    n = NT1 + 1
    w = vio.synth.make_window(n, seed=18)
    c = well_posed(vio, hip_lib, w)
    c.covariance(w)
    l = NT1 - 1
    e = int(np.nonzero(w.lm == l)[0][1])                           # its second edge
    bad = w.copy()
    bad.host = np.array(w.host)
    bad.host[e] = (bad.host[e] + 1) % vio.NUM_FRAMES
    P, L = sentinels(n)
    with pytest.raises(vio.VioError) as ei:
        c._cov.compute(bad, "fix_oldest", pose_cov=P, lm_out=L)
    assert ei.value.status == -1, str(ei.value)
    assert "landmark %d has observations with different host frames" % l in str(ei.value), str(ei.value)
    assert np.all(P == 7.0) and np.all(L == 7.0)
    P1, L1 = c.covariance(w)
    assert np.all(np.isfinite(P1)) and np.all(L1 > 0)


def test_an_xyz_landmark_the_list_has_no_edge_of(vio, hip_lib):
    """k_cov_landmarks<3>: H_ll = 0 fails Sylvester's criterion at its first minor; landmark LmNT<3> is the second workgroup's only
    live lane."""
    n = NT3 + 1
    w = vio.synth.make_window_xyz(n, seed=18)
    c = well_posed(vio, hip_lib, w)
    P0, L0 = c.covariance(w)
    bare = rr.take_edges(w, w.lm != NT3)
    P, L = np.full((cr.PD, cr.PD), 7.0), np.full((n, 3, 3), 7.0)
    with pytest.raises(vio.VioError) as ei:
        c._cov.compute(bare, "fix_oldest", pose_cov=P, lm_out=L)
    assert ei.value.status == -3 and "landmark %d: its information" % NT3 in str(ei.value), str(ei.value)
    assert np.all(P == 7.0) and np.all(L == 7.0)
    P1, L1 = c.covariance(w)
    assert np.array_equal(P1, P0) and np.array_equal(L1, L0)
