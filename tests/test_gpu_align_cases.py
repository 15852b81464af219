"""GPU parity of the alignment kernels (align.hip: k_align_resid, k_align_reduce, k_align_update, k_align_depth_update,
k_align_pack_anchors, k_align_points) on every row, partial, view, tree, clamp and tie edge of tests/align_cases.py,
against the float64 oracle (oracle/align_oracle.loss_and_grads); tests/test_oracle_align_cases.py pins the inputs.

What is observed: one Adam step from zero moments leaves m = 0.1 g and v = 0.1 g^2, so the kernels' gradient is read
from `_adam_m` / `_adam_v` (`_adam_m_core` for the core depths); the camera table and the points come from a run with no
iteration.  Bounds: per parameter group (the 11 columns of the optimiser's state; the trainable ones of the stage), the
error over the group's float64 maximum is at most 4 x the float32 oracle's own on that case, floor 5e-5; loss rtol 2e-5;
table and points 4 x the float32 oracle's, floor 1e-5.  Every figure is printed before it is asserted
(`FIG <case> <group> <error> <bound>`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import align_cases as ac
from oracle import align_oracle as ao
from test_gpu_align import run_hip

LR = {1: 0.07, 2: 0.014}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b, keys):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


RES_KEYS = ("intrinsics", "cam2w", "depthmaps", "pts3d", "losses", "_adam_m", "_adam_v", "_flags")


def check_group(tag, got, ref64, scale, bound):
    """`got` against `ref64`, error over `scale` at most `bound`; a group that is exactly zero in float64 is exactly zero"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), tag
    if scale == 0.0:
        assert not got.any(), tag
        return 0.0
    err = float(np.abs(got - ref64).max()) / scale
    print("FIG %s %.3e %.3e" % (tag, err, bound))
    assert err <= bound, (tag, err, bound)
    return err / bound


def check_moments(tag, case, res, R, groups=None, bounds=None):
    """m = 0.1 g and v = 0.1 g^2 of the trainable groups; the others keep no moment"""
    C = case.C
    m, v = ac.moment_groups(res["_adam_m"], C), ac.moment_groups(res["_adam_v"], C)
    groups = case.trainable() if groups is None else groups
    bounds = ac.grad_bounds(R, groups, case.grad_floor) if bounds is None else bounds
    for k, c in ac.GROUPS:
        if (k, c) not in groups:
            assert not m[k][:, c].any() and not v[k][:, c].any(), (tag, k, c)
            continue
        scale, yard, bound = bounds[(k, c)]
        g64 = R["f64"]["grads"][k].reshape(C, -1)[:, c]
        check_group(f"{tag} {k}[{c}]", 10.0 * m[k][:, c], g64, scale, bound)
        e = bound * scale
        slack = 0.1 * (2 * np.abs(g64) * e + e * e) + 1e-6 * 0.1 * g64 * g64 + 1e-30
        assert (np.abs(v[k][:, c].astype(np.float64) - 0.1 * g64 * g64) <= slack).all(), (tag, "v", k, c)


def check_first_step(tag, case, par, R, stage):
    """one Adam step from zero moments moves a parameter by lr g / (|g| + 1e-8); frozen parameters keep their bits"""
    lr = LR[stage]
    for k in ac.PARAM_KEYS:
        p0 = case.params[k].reshape(case.C, -1)
        p1 = np.asarray(par[k]).reshape(case.C, -1)
        for c in range(ac.WIDTH[k]):
            if (k, c) not in case.trainable():
                assert np.array_equal(bits(p0[:, c]), bits(p1[:, c])), (tag, k, c)
            elif k != "quats":    # (the quaternion is renormalised after its step)
                g = R["f64"]["grads"][k].reshape(case.C, -1)[:, c]
                big = np.abs(g) > max(1e-4, 1e-3 * float(np.abs(g).max()))
                want = -lr * np.sign(g[big])
                got = p1[big, c].astype(np.float64) - p0[big, c]
                assert (np.abs(got - want) <= 2e-4 * lr + 1e-6).all(), (tag, k, c)


def hip(case, n1, n2, params=None, **over):
    kw = dict(case.kw); kw.update(over)
    return run_hip(case.flat, niter1=n1, niter2=n2, prev_params=params if params is not None else case.params, **kw)


@pytest.mark.parametrize("name", ac.SINGLE)
def test_case(name):
    case = ac.get(name)
    R = ac.reference(name)
    C = case.C
    # ---- no iteration: the camera table and the points
    res0, par0 = hip(case, 0, 0)
    for k, (scale, yard, bound) in ac.table_bounds(R).items():
        got = res0[k][..., :3, :] if k == "cam2w" else res0[k]
        ref = R["f64"][k][..., :3, :] if k == "cam2w" else R["f64"][k]
        check_group(f"{name} {k}", got, ref, scale, bound)
    for k in ac.PARAM_KEYS:
        assert np.array_equal(bits(par0[k]), bits(case.params[k].reshape(par0[k].shape))), k
    if "fclip" in case.expect:      # the table holds the clamped focal
        diag = np.linalg.norm(case.flat["imsizes"].astype(np.float64), axis=1)
        np.testing.assert_allclose(res0["intrinsics"][[1, 2], 0, 0], [0.25 * diag[1], 10 * diag[2]], rtol=2e-7)
    # ---- one step of the case's stage: loss, gradient, moments
    n1, n2 = case.iters["niter1"], case.iters["niter2"]
    res, par = hip(case, n1, n2)
    assert res["losses"].shape == (1,) and res["_flags"][1] == 0
    if case.rows == 0:
        assert res["losses"][0] == 0
        for k in ("pps", "log_focals", "trans", "log_sizes"):
            assert np.array_equal(bits(par[k]), bits(par0[k])), k
        np.testing.assert_allclose(par["quats"], par0["quats"], rtol=0, atol=1.2e-7)   # renormalised: at most one ulp
    else:
        print("FIG %s loss %.3e %.3e" % (name, abs(res["losses"][0] / R["f64"]["loss"] - 1), ac.LOSS_RTOL))
        np.testing.assert_allclose(res["losses"][0], R["f64"]["loss"], rtol=ac.LOSS_RTOL)
    check_moments(name, case, res, R)
    if case.rows:
        check_first_step(name, case, par, R, case.stage)
    if "fclip" in case.expect and case.stage == 2:      # beyond a focal limit the log-focal gradient is exactly zero
        m = ac.moment_groups(res["_adam_m"], C)["log_focals"][:, 0]
        assert m[1] == 0 and m[2] == 0 and m[0] != 0 and m[3] != 0
        assert par["log_focals"][1] == case.params["log_focals"][1] and par["log_focals"][2] == case.params["log_focals"][2]
    if case.kw.get("opt_depth"):
        g64, g32 = R["f64"]["grads"]["core_depth"], R["f32"]["grads"]["core_depth"]
        scale, yard, bound = ac.group_bound(g64, g32, ac.GRAD_FLOOR)
        got = 10.0 * res["_adam_m_core"]
        check_group(f"{name} core_depth", got, g64, scale, bound)
        # the zero pattern is the float64 one: a core depth no row reads (or only rows clipped in u, v or z) gets none
        assert np.array_equal(got == 0, g64 == 0) and (g64[ac.depth_reads(case) == 0] == 0).all() and (g64 != 0).any()
    # ---- the results of a run belong to the start of its last iteration: here, the table of the run without one
    same_bits(res, res0, ("intrinsics", "cam2w", "depthmaps", "pts3d"))
    # ---- bit-reproducible
    res2, par2 = hip(case, n1, n2)
    same_bits(res, res2, RES_KEYS)
    same_bits(par, par2, ac.PARAM_KEYS)
    if case.kw.get("opt_depth"):
        same_bits(res, res2, ("_adam_m_core",)); same_bits(par, par2, ("core_depth",))


def test_more_views_than_the_update_workgroup_holds_are_refused(monkeypatch):
    """C = 257 > MAXC: ST3R_ERR_INVALID, and nothing is written -- every device buffer handed to the library (the
    parameters, the work and result buffers, the problem's arrays) holds afterwards the bits it held when its pointer
    was taken; the context serves the next call as before."""
    from starst3r_amd import ops
    small = ac.get("rows_65_s1")
    before = hip(small, 1, 0)
    root, edges = ac.path_tree(257)
    flat = ac.build(257, [(0, 1, 10)], tree=(root, edges), seed=3)
    seen, real_p = [], ops._p

    def recording_p(t, dtype=torch.float32):
        if t is not None and t.numel():
            if t.dtype == torch.float32:
                t.view(torch.int32).bitwise_and_(0x7fffff).bitwise_or_(0x3f000000)   # defined bits in what torch.empty left
            seen.append((t, t.clone()))
        return real_p(t, dtype)
    monkeypatch.setattr(ops, "_p", recording_p)
    with pytest.raises(ValueError, match="invalid argument"):
        run_hip(flat, niter1=1, niter2=0, prev_params=ac.generic_params(flat, 3))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(seen) >= 25                                   # problem arrays, five parameter tensors, work, cam, pts, losses
    for t, was in seen:
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    after = hip(small, 1, 0)
    same_bits(before[0], after[0], RES_KEYS); same_bits(before[1], after[1], ac.PARAM_KEYS)


def five(par):
    return {k: np.asarray(par[k]) for k in ac.PARAM_KEYS}


def pair(case, params, stage, core=None):
    return {"f64": ac.evaluate(case, torch.float64, params=params, core=core, stage=stage),
            "f32": ac.evaluate(case, torch.float32, params=params, core=core, stage=stage)}


def combine(Ra, Rb, groups, C):
    """expected moments after two steps from zero: m = 0.09 g1 + 0.1 g2, v = 0.09 g1^2 + 0.1 g2^2, and the gradient
    bounds of the two evaluations carried through those sums -> {(key, column): (m, e_m, v, e_v)}"""
    ba, bb = ac.grad_bounds(Ra, groups), ac.grad_bounds(Rb, groups)
    out = {}
    for k, c in groups:
        g1 = Ra["f64"]["grads"][k].reshape(C, -1)[:, c]; g2 = Rb["f64"]["grads"][k].reshape(C, -1)[:, c]
        e1, e2 = ba[(k, c)][0] * ba[(k, c)][2], bb[(k, c)][0] * bb[(k, c)][2]
        out[(k, c)] = (0.09 * g1 + 0.1 * g2, 0.09 * e1 + 0.1 * e2, 0.09 * g1 * g1 + 0.1 * g2 * g2,
                       0.09 * (2 * np.abs(g1) * e1 + e1 * e1) + 0.1 * (2 * np.abs(g2) * e2 + e2 * e2))
    return out


@pytest.mark.parametrize("name", ["steps_2000", "steps_33wg"])
def test_second_step_and_stage_change(name):
    """(1, 0) gives p1 (bit-reproducible, so well defined).  (2, 0): the second step's moments are the two gradients'
    sums -- magnitudes the first step (lr sign(g)) hides -- and its parameter step follows Adam's bias corrections of
    step 2.  (1, 1): stage 2 starts a fresh optimiser at p1 -- all 11 groups hold 0.1 g / 0.1 g^2 of ITS gradient, nothing
    of stage 1."""
    case = ac.get(name)
    C = case.C
    assert case.shape[1] == case.expect["n_part"]
    resA, parA = hip(case, 1, 0)
    p0, p1 = case.params, five(parA)
    Ra, Rb = pair(case, p0, 1), pair(case, p1, 1)
    check_moments(f"{name} step1", case, resA, Ra)
    groups = case.trainable()
    resB, parB = hip(case, 2, 0)
    m, v = ac.moment_groups(resB["_adam_m"], C), ac.moment_groups(resB["_adam_v"], C)
    want = combine(Ra, Rb, groups, C)
    for (k, c), (wm, em, wv, ev) in want.items():
        err = np.abs(m[k][:, c] - wm).max(); errv = (np.abs(v[k][:, c] - wv) / (ev + 1e-6 * wv)).max()
        print("FIG %s step2 %s[%d] m %.3e %.3e v (error over bound) %.3e 1" % (name, k, c, err, em, errv))
        assert err <= em + 1e-7 * np.abs(wm).max() and (np.abs(v[k][:, c] - wv) <= ev + 1e-6 * wv).all(), (k, c)
    for k in ("pps", "log_focals"):
        assert not m[k].any() and not v[k].any()
        assert np.array_equal(bits(parB[k]), bits(np.asarray(p0[k]).reshape(parB[k].shape)))
    # the parameter step of step 2: lr(1 / 2) / (1 - 0.9^2) * m / (sqrt(v) / sqrt(1 - 0.9^2) + 1e-8), where the moments are
    # well away from zero; the error of m / sqrt(v) follows from the bounds above
    lr2 = float(ao.cosine_schedule(0.5, LR[1], 0))
    for k in ("trans", "log_sizes"):
        for c in range(ac.WIDTH[k]):
            wm, em, wv, ev = want[(k, c)]
            big = np.abs(wm) > 0.05 * np.abs(wm).max()
            step = lr2 / 0.19 * wm / (np.sqrt(wv) / np.sqrt(0.19) + 1e-8)
            rel = em / np.abs(wm[big]) + 0.5 * ev[big] / wv[big] + 1e-5
            got = np.asarray(p1[k]).reshape(C, -1)[big, c].astype(np.float64) - parB[k].reshape(C, -1)[big, c]
            assert (np.abs(got - step[big]) <= rel * np.abs(step[big]) + 1e-6).all(), (k, c)
    # stage change
    resC, parC = hip(case, 1, 1)
    Rc = pair(case, p1, 2)
    rz, u, v2, d = ac.rows2d(case, Rc["f64"])
    assert ac.threshold_margin(rz, u, v2) > 1e-3 and (d > 1e-3).all()       # (p1 comes from the GPU: checked here)
    check_moments(f"{name} stage2", case, resC, Rc, groups=list(ac.GROUPS))
    np.testing.assert_allclose(resC["losses"][1], Rc["f64"]["loss"], rtol=ac.LOSS_RTOL)
    assert np.array_equal(bits(resC["losses"][:1]), bits(resA["losses"][:1]))


def test_core_depth_moments_over_two_steps_and_the_stage_change():
    """opt_depth: (1, 1) -- the core depths' first moments at the first step of stage 2 are 0.1 x their gradient at p1;
    (0, 2) -- the second step reads the STEPPED core depths (the anchors are repacked after a depth step): m = 0.09 g1 +
    0.1 g2 with g2 evaluated at the parameters and core depths the first step left."""
    case = ac.get("steps_depth")
    C = case.C
    zero = ac.depth_reads(case) == 0
    core_bound = lambda R: ac.group_bound(R["f64"]["grads"]["core_depth"], R["f32"]["grads"]["core_depth"], ac.GRAD_FLOOR)
    # stage change
    _, parS = hip(case, 1, 0)
    resC, _ = hip(case, 1, 1)
    Rc = pair(case, five(parS), 2)
    scale, yard, bound = core_bound(Rc)
    check_group("steps_depth stage2 core_depth", 10.0 * resC["_adam_m_core"], Rc["f64"]["grads"]["core_depth"], scale, bound)
    assert np.array_equal(resC["_adam_m_core"] == 0, Rc["f64"]["grads"]["core_depth"] == 0)
    check_moments("steps_depth stage2", case, resC, Rc, groups=list(ac.GROUPS))
    # two steps of stage 2
    resA, parA = hip(case, 0, 1)
    Ra = pair(case, case.params, 2)
    Rb = pair(case, five(parA), 2, core=parA["core_depth"])
    assert not np.array_equal(parA["core_depth"][~zero], hip(case, 0, 0)[1]["core_depth"][~zero])
    resB, parB = hip(case, 0, 2)
    sa, _, ba = core_bound(Ra); sb, _, bb = core_bound(Rb)
    want = 0.09 * Ra["f64"]["grads"]["core_depth"] + 0.1 * Rb["f64"]["grads"]["core_depth"]
    e = 0.09 * sa * ba + 0.1 * sb * bb
    err = float(np.abs(resB["_adam_m_core"] - want).max())
    print("FIG steps_depth step2 core_depth m %.3e %.3e" % (err, e))
    assert err <= e + 1e-7 * np.abs(want).max()
    assert np.array_equal(resB["_adam_m_core"] == 0, want == 0) and (want[zero] == 0).all()
    groups = list(ac.GROUPS)
    m = ac.moment_groups(resB["_adam_m"], C)
    for (k, c), (wm, em, wv, ev) in combine(Ra, Rb, groups, C).items():
        assert np.abs(m[k][:, c] - wm).max() <= em + 1e-7 * np.abs(wm).max(), (k, c)


def test_schedule_callable_equals_the_built_in_cosine():
    """equal learning rates (tests/test_oracle_align_cases.py pins that they are) give equal bits"""
    case = ac.get("steps_2000")
    a = hip(case, 3, 1, lr1=0.0625, lr2=0.015625)
    b = hip(case, 3, 1, lr1=0.0625, lr2=0.015625, schedule=ao.cosine_schedule)
    same_bits(a[0], b[0], RES_KEYS); same_bits(a[1], b[1], ac.PARAM_KEYS)
    c = hip(case, 3, 1, lr1=0.0625, lr2=0.015625, schedule=ao.linear_schedule)
    assert not np.array_equal(bits(a[1]["trans"]), bits(c[1]["trans"]))


@pytest.mark.parametrize("wgs,stage", [(10, 2), (33, 1)])
def test_nan_loss_stops_the_run(wgs, stage):
    """The first loss is NaN: it is stored, the flag is set, every later launch returns early (their losses stay 0) --
    with k_align_update adding the partials itself (10 workgroups) and behind k_align_reduce (33).  The chain cache and the
    accumulators are shared scratch of the context: a clean problem run next gives the bits it gave before."""
    clean, bad, params = ac.nan_case(wgs, stage)
    it = dict(niter1=3, niter2=0) if stage == 1 else dict(niter1=0, niter2=3)
    before = run_hip(clean, prev_params=params, **it)
    assert np.isfinite(before[0]["losses"]).all() and (before[0]["losses"] > 0).all() and before[0]["_flags"][1] == 0
    res, par = run_hip(bad, prev_params=params, **it)
    L = res["losses"]
    assert L.shape == (3,) and np.isnan(L[0]) and L[1] == 0 and L[2] == 0
    assert res["_flags"][1] == 1
    after = run_hip(clean, prev_params=params, **it)
    same_bits(before[0], after[0], RES_KEYS); same_bits(before[1], after[1], ac.PARAM_KEYS)
