"""The batched non-keyframe PnP on the GPU (include/vio_pnp.h) against the numpy restatement (tests/pnp_reference.py, order "wave64").

The rule is that of test_gpu_sfm.py: statuses, point counts and iteration counts must be identical; each frame's pose must lie inside
10x the restatement's own spread when every image point of the frame moves by one ulp (two such perturbations), plus 1e-13 of the
quantity's size.  A frame whose iteration count already changes under that perturbation in the restatement is undecidable and is
skipped; at most 2 of the 20 fixture frames may be (tests/test_pnp_reference.py checks on the CPU that the committed seeds give 0).

End to end (sfm_batch -> frames_batch -> all_frames_to_init_items -> initialize_batch) the GPU chain's scale (relative), gravity
(relative to |g|) and the velocities of all 21 frames (relative to the largest speed, at least 1 m/s) are held to the ground truth on
every window.  On the noise-free variants the bound is test_gpu_init_stream.py's 1e-3 on the scale, which that file applies where the
visual input is noise-free; gravity and the velocities are held to the same 1e-3: the three come out of one linear system.  Measured
on an MI355X: synthetic 4.1e-5 / 6.1e-6 / 4.2e-5, MH_05 4.4e-8 / 2.8e-9 / 4.2e-8.  On the 0.1 px windows, where the keyframes' SfM
alone moves the scale by more than 1e-3, the bar is 10 x the error the chain of the three CPU restatements itself shows on that window
(the rule of tests/test_pnp_reference.py), measured on the CPU:
    synthetic, 0.1 px   1.613e-3 / 1.678e-3 / 2.388e-3     bars 1.6e-2 / 1.7e-2 / 2.4e-2
    MH_05, 0.1 px       3.757e-3 / 2.938e-4 / 2.490e-3     bars 3.8e-2 / 2.9e-3 / 2.5e-2
The velocities are read from x (3 per frame of all_image_frame): the reference's own Vs[kv] = x.segment<3>(kv * 3) indexes x by the
keyframe counter, which the alignment library reproduces.
The GPU and CPU chains are held to 2e-2, the tolerance test_gpu_sfm_stream.py uses between two runs of its pipeline, and, much
tighter, to 10 x the CPU chain's own spread when every image point (the keyframes' and the non-keyframes') moves by one ulp (two such
perturbations), plus 1e-13: measured spreads are 1e-14 to 1e-12, the GPU chain's distance 6e-14 to 7e-13.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_reference as ir  # noqa: E402
import pnp_reference as pr  # noqa: E402
import sfm_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("status", "fail_frame", "Q", "T", "frame_status", "iterations", "n_used", "cost")


@pytest.fixture(scope="module")
def pnp_lib(vio, hip_lib):
    return vio.load_pnp()


def _bits(d, frames=None):
    sel = slice(None) if frames is None else frames
    return [np.asarray(d[k])[sel].tobytes() if np.ndim(d[k]) else np.asarray(d[k]).tobytes() for k in KEYS]


def _frame_bits(d, k):
    return [np.asarray(d[key])[k].tobytes() for key in ("Q", "T", "frame_status", "iterations", "n_used", "cost")]


def _compare(got, item, name, seed=5):
    """The device's window against the restatement's; returns the number of undecidable frames."""
    ref = pr.frames(item)
    rng = np.random.RandomState(seed)
    runs = [pr.frames(pr.perturb_ulp(item, rng)) for _ in range(2)]
    assert (got["status"], got["fail_frame"]) == (ref["status"], ref["fail_frame"]), name
    assert np.array_equal(got["frame_status"], ref["frame_status"]) and np.array_equal(got["n_used"], ref["n_used"]), name
    skipped = 0
    for k in range(len(ref["Q"])):
        if any(r["iterations"][k] != ref["iterations"][k] for r in runs):
            skipped += 1
            continue
        assert got["iterations"][k] == ref["iterations"][k], (name, k, got["iterations"][k], ref["iterations"][k])
        if ref["frame_status"][k] != pr.OK:
            assert np.all(np.isnan(got["Q"][k])) and np.all(np.isnan(got["T"][k])) and np.isnan(got["cost"][k]), (name, k)
            continue
        for key in ("Q", "T", "cost"):
            sp = max(float(np.max(np.abs(r[key][k] - ref[key][k]))) for r in runs)
            bar = 10.0 * sp + 1e-13 * max(1.0, float(np.max(np.abs(ref[key][k]))))
            err = float(np.max(np.abs(got[key][k] - ref[key][k])))
            print("%-16s frame %2d %-4s err %.3e  bar %.3e  n %d  it %d" % (name, k, key, err, bar, ref["n_used"][k], ref["iterations"][k]))
            assert err <= bar, (name, k, key, err, bar)
    return skipped


def test_frames_match_restatement(vio, pnp_lib):
    items = [pr.fixture("syn")["item"], pr.fixture("mh")["item"]]
    got = pnp_lib.create().frames_batch(items)
    skipped = sum(_compare(g, it, name) for g, it, name in zip(got, items, ("syn", "mh")))
    print("undecidable frames:", skipped, "of 20")
    assert skipped <= 2 and all(len(g["Q"]) == 10 and g["status"] == 0 for g in got)


def _usable(item, k):
    off = item["obs_offset"]
    return np.nonzero(item["valid"][item["obs_point"][off[k]:off[k + 1]]])[0]


def test_lane_boundaries(vio, pnp_lib):
    h = pnp_lib.create()
    item = pr.fixture("syn")["item"]
    u = _usable(item, 9)
    assert len(u) >= 129
    cuts = [(n, pr.frame_item(item, 9, u[:n])) for n in (6, 63, 64, 65, 128, 129)]
    big = pr.synthetic_frame(pr.MAX_POINTS, 3)
    flat = pr.synthetic_frame(100, 4)
    batch = [c for _, c in cuts] + [big, flat]
    got = h.frames_batch(batch)
    for (n, c), g in zip(cuts, got):
        assert g["n_used"][0] == n and g["status"] == 0
        assert _compare(g, c, "cut %d" % n) == 0
    assert got[6]["n_used"][0] == pr.MAX_POINTS and _compare(got[6], big, "max points") == 0
    assert _compare(got[7], flat, "flat") == 0
    # every second observation's point invalid == those observations removed, bit for bit
    k = 7
    off = item["obs_offset"]
    op = item["obs_point"][off[k]:off[k + 1]]
    valid = item["valid"].copy()
    valid[op[1::2]] = False
    a = h.frames_batch([pr.frame_item(dict(item, valid=valid), k)])[0]
    keep = np.nonzero(valid[op])[0]
    assert 0 < len(keep) < len(_usable(item, k)) and len(keep) > 64
    b = h.frames_batch([pr.frame_item(item, k, keep)])[0]
    assert a["n_used"][0] == len(keep) and a["status"] == 0 and _bits(a) == _bits(b)
    assert _compare(a, pr.frame_item(dict(item, valid=valid), k), "every second invalid") == 0


def _failing(item, k=4, n=5):
    """The item with frame k cut to its first n usable observations."""
    off = item["obs_offset"]
    op, ob, o = [], [], [0]
    for f in range(len(item["guess_key"])):
        keep = _usable(item, f)[:n] if f == k else np.arange(off[f + 1] - off[f])
        op.append(item["obs_point"][off[f]:off[f + 1]][keep]); ob.append(item["obs_pts"][off[f]:off[f + 1]][keep]); o.append(o[-1] + len(keep))
    return dict(item, obs_offset=np.array(o, dtype=np.int64), obs_point=np.concatenate(op), obs_pts=np.concatenate(ob))


def _no_frames(item):
    return dict(item, guess_key=np.zeros(0, dtype=np.int32), obs_offset=np.zeros(1, dtype=np.int64), obs_point=np.zeros(0, dtype=np.int32),
                obs_pts=np.zeros((0, 2)))


def test_batch_properties(vio, pnp_lib):
    h = pnp_lib.create()
    syn, mh = pr.fixture("syn")["item"], pr.fixture("mh")["item"]
    # a 21-frame window (10 non-keyframes), a window without frames, a 1-frame window, a window with a failing frame in the middle
    batch = [syn, _no_frames(syn), pr.frame_item(mh, 6), _failing(mh)]
    alone = [h.frames_batch([it])[0] for it in batch]
    for order in (batch, batch[::-1]):
        out = h.frames_batch(order)
        again = h.frames_batch(order)
        ref = alone if order is batch else alone[::-1]
        for o, a, r in zip(out, again, ref):
            assert _bits(o) == _bits(a) == _bits(r)
    assert alone[1]["status"] == 0 and alone[1]["fail_frame"] == -1 and alone[1]["Q"].shape == (0, 4)
    # the only frame of its window, and the 3rd of 10 (another wavefront of the workgroup): the same bits
    one = h.frames_batch([pr.frame_item(syn, 2)])[0]
    assert _frame_bits(one, 0) == _frame_bits(alone[0], 2)
    # outcomes: the 5-point frame is reported, the frames after it are still solved and equal their solo results
    f = alone[3]
    whole = h.frames_batch([mh])[0]
    assert (f["status"], f["fail_frame"]) == (pr.FAIL_FEW_POINTS, 4) and f["n_used"][4] == 5 and np.all(np.isnan(f["Q"][4]))
    for k in (0, 3, 5, 9):
        assert f["frame_status"][k] == 0 and _frame_bits(f, k) == _frame_bits(whole, k)
        assert _frame_bits(f, k) == _frame_bits(h.frames_batch([pr.frame_item(mh, k)])[0], 0)
    assert _compare(f, batch[3], "failing") <= 1
    six = h.frames_batch([_failing(mh, 4, 6)])[0]
    assert six["status"] == 0 and six["n_used"][4] == 6 and np.all(np.isfinite(six["Q"][4]))
    h.set_config(min_points=7)
    assert h.frames_batch([_failing(mh, 4, 6)])[0]["fail_frame"] == 4
    h.set_config()
    # a NaN observation: that window only; a point in the guess camera's z = 0 plane: an outcome
    ob = syn["obs_pts"].copy()
    ob[syn["obs_offset"][2] + 1, 0] = np.nan
    flat = pr.synthetic_frame(8, 1)
    flat["points"][3, 2] = 0.0
    out = h.frames_batch([mh, dict(syn, obs_pts=ob), flat, syn])
    assert [o["status"] for o in out] == [0, pr.NOT_FINITE, pr.FAIL_NO_POSE, 0]
    assert np.all(np.isnan(out[1]["Q"])) and np.all(out[1]["frame_status"] == pr.NOT_FINITE) and out[1]["fail_frame"] == -1
    assert out[2]["fail_frame"] == 0 and out[2]["iterations"][0] == 0
    assert _bits(out[0]) == _bits(whole) and _bits(out[3]) == _bits(alone[0])


def _raw_call(pnp_lib, h, item, null=None, count=1):
    """frames_batch through the raw entry point with sentinel-filled outputs; returns (status, the outputs untouched?)."""
    from vio_amd import pnp
    pk = pnp._Packed([item])
    if null:
        setattr(pk.items[0], null, None)
    nf = max(pk.total, 40)
    res = (pnp.VioPnpResult * 1)()
    res[0].status, res[0].fail_frame = 77, 77
    Q, T = np.full((nf, 4), 7.5), np.full((nf, 3), 7.5)
    info = (pnp.VioPnpFrameInfo * nf)()
    for i in range(nf):
        info[i].status = 77
    st = pnp_lib.fn["frames_batch"](h.h, C.c_int32(count), C.addressof(pk.items), C.addressof(res), Q.ctypes.data, T.ctypes.data,
                                    C.addressof(info))
    untouched = res[0].status == 77 and res[0].fail_frame == 77 and np.all(Q == 7.5) and np.all(T == 7.5) and all(info[i].status == 77 for i in range(nf))
    return st, untouched


def test_count_zero_and_bad_arguments(vio, pnp_lib):
    h = pnp_lib.create()
    assert h.frames_batch([]) == []
    item = pr.fixture("syn")["item"]
    good = h.frames_batch([item])[0]
    n = len(item["obs_point"])
    gk33 = np.zeros(33, dtype=np.int32)
    off33 = np.concatenate([item["obs_offset"], np.full(23, n)]).astype(np.int64)
    op_bad = item["obs_point"].copy(); op_bad[5] = len(item["points"])
    op_neg = item["obs_point"].copy(); op_neg[0] = -1
    gk_bad = item["guess_key"].copy(); gk_bad[3] = 11
    many = pr.synthetic_frame(pr.MAX_POINTS + 1, 2)
    cases = [("n_frames = 33", dict(item, guess_key=gk33, obs_offset=off33), None),
             ("obs_point out of range", dict(item, obs_point=op_bad), None), ("obs_point negative", dict(item, obs_point=op_neg), None),
             ("guess_key out of range", dict(item, guess_key=gk_bad), None), ("4097 observations", many, None)]
    cases += [("NULL " + f, item, f) for f in ("points", "key_Q", "key_T", "guess_key", "obs_offset", "obs_point", "obs_pts")]
    for name, it, null in cases:
        st, untouched = _raw_call(pnp_lib, h, it, null)
        assert st == -1 and untouched, name
        assert "window 0" in h.last_error(), (name, h.last_error())
    empty = dict(item, obs_offset=np.zeros(11, dtype=np.int64), obs_point=np.zeros(0, dtype=np.int32), obs_pts=np.zeros((0, 2)))
    assert h.frames_batch([empty])[0]["status"] == pr.FAIL_FEW_POINTS
    st, untouched = _raw_call(pnp_lib, h, empty, "points")          # no observations: points is still required while n_points > 0
    assert st == -1 and untouched and "window 0" in h.last_error()
    st, untouched = _raw_call(pnp_lib, h, item, count=-1)
    assert st == -1 and untouched
    st, untouched = _raw_call(pnp_lib, h, item, count=0)
    assert st == 0 and untouched
    fn = pnp_lib.fn["frames_batch"]
    assert fn(h.h, C.c_int32(1), None, None, None, None, None) == -1
    with pytest.raises(vio.VioError) as e:
        h.frames_batch([item, dict(item, guess_key=gk_bad)])
    assert e.value.status == -1 and "window 1" in str(e.value)
    with pytest.raises(vio.VioError):
        h.set_config(min_points=2)
    assert _bits(h.frames_batch([item])[0]) == _bits(good)         # the handle is unharmed
    t = h.timing()
    assert t["kernel_ms"] > 0 and t["total_ms"] >= t["kernel_ms"]


# against the ground truth (scale, gravity, velocities; see the module docstring)
TRUTH_BARS = {("syn", False): (1e-3, 1e-3, 1e-3), ("mh", False): (1e-3, 1e-3, 1e-3),
              ("syn", True): (1.6e-2, 1.7e-2, 2.4e-2), ("mh", True): (3.8e-2, 2.9e-3, 2.5e-2)}


def _truth_errors(st, win, l, ric, G, r, it):
    _, _, _, s_true = sr.ground_truth(st, win["key_frames"], l, [])
    Rcl = st.R[win["key_frames"][l]] @ ric
    g_true = Rcl.T @ np.array([0.0, 0.0, G])
    v_true = np.stack([st.V[f] for f in win["frames"]])
    v_est = np.stack([Rcl @ it["R"][k] @ r["x"][3 * k:3 * k + 3] for k in range(len(win["frames"]))])
    return abs(r["s"] / s_true - 1.0), float(np.abs(r["g"] - g_true).max()) / G, float(np.abs(v_est - v_true).max()) / max(1.0, float(np.abs(v_true).max()))


@pytest.mark.parametrize("which,noisy", [("syn", False), ("mh", False), ("syn", True), ("mh", True)])
def test_initial_structure_end_to_end(vio, hip_lib, oracle_lib, pnp_lib, which, noisy):
    fx = pr.fixture(which, noisy)
    st, win = fx["stream"], fx["win"]
    ric, tic = vio.synth.quat_to_rot(st.ext[3:7]), st.ext[0:3].copy()
    G = float(getattr(st, "g_norm", vio.synth.G_NORM))
    noise = dict(getattr(st, "noise", None) or {})
    # the GPU chain
    sfm = vio.load_sfm().create().sfm_batch([win["sfm_item"]])
    assert sfm[0]["status"] == 0
    items = vio.pnp_items_from_sfm(sfm, [win["sfm_item"]], [win["all_frames"]])
    pnp = pnp_lib.create().frames_batch(items)
    assert pnp[0]["status"] == 0 and len(pnp[0]["Q"]) == 10
    init_items = vio.all_frames_to_init_items(sfm, pnp, ric, [win["pres"]], [win["is_key"]])
    assert init_items[0]["R"].shape == (21, 3, 3) and sum(init_items[0]["is_key"]) == 11
    g = vio.load_init().create().initialize_batch(init_items, [win["intervals"]], vio.load_imu().create(), tic, G, noise)[0]
    assert g["status"] == 0 and g["n_key"] == 11 and g["s"] > 0
    # the CPU chain: the three restatements
    cpnp = pr.frames(fx["item"])
    citems = vio.all_frames_to_init_items([fx["sfm"]], [cpnp], ric, [win["pres"]], [win["is_key"]])
    c = ir.make_aligner(oracle_lib)(citems, [win["intervals"]], tic, G, noise)[0]
    assert c["status"] == 0
    assert sfm[0]["rel"]["l"] == fx["sfm"]["rel"]["l"]
    vmax = max(1.0, float(np.abs(c["speed_bias"][:, 0:3]).max()))
    ds, dg, dv = abs(g["s"] / c["s"] - 1.0), float(np.abs(g["g"] - c["g"]).max()), float(np.abs(g["speed_bias"][:, 0:3] - c["speed_bias"][:, 0:3]).max())
    print(which, noisy, "GPU vs CPU chain: s %.3e g %.3e v %.3e" % (ds, dg / G, dv / vmax))
    assert ds <= 2e-2 and dg <= 2e-2 * G and dv <= 2e-2 * vmax
    rng = np.random.RandomState(7)
    sp = np.zeros(3)
    for _ in range(2):          # the CPU chain's own spread under one ulp of every image point
        item1 = sr.perturb_ulp(win["sfm_item"], rng)
        sfm1 = sr.sfm(item1)
        pnp1 = pr.frames(pr.perturb_ulp(vio.pnp_items_from_sfm([sfm1], [item1], [win["all_frames"]])[0], rng))
        it1 = vio.all_frames_to_init_items([sfm1], [pnp1], ric, [win["pres"]], [win["is_key"]])
        p = ir.make_aligner(oracle_lib)(it1, [win["intervals"]], tic, G, noise)[0]
        assert p["status"] == 0
        sp = np.maximum(sp, [abs(p["s"] / c["s"] - 1.0), float(np.abs(p["g"] - c["g"]).max()) / G,
                             float(np.abs(p["speed_bias"][:, 0:3] - c["speed_bias"][:, 0:3]).max()) / vmax])
    print(which, noisy, "CPU chain's one-ulp spread: s %.3e g %.3e v %.3e" % tuple(sp))
    assert ds <= 10.0 * sp[0] + 1e-13 and dg / G <= 10.0 * sp[1] + 1e-13 and dv / vmax <= 10.0 * sp[2] + 1e-13
    es, eg, ev = _truth_errors(st, win, fx["sfm"]["rel"]["l"], ric, G, g, init_items[0])
    print(which, noisy, "GPU chain vs ground truth: s %.3e g %.3e v %.3e" % (es, eg, ev))
    bs, bg, bv = TRUTH_BARS[(which, noisy)]
    assert es <= bs and eg <= bg and ev <= bv, (es, eg, ev)
