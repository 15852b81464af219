"""Spherical harmonics of degree 0..3 on the GPU: st3r_ctx_set_sh_degree through st3r_gs_project_sh, st3r_gs_project_sh_bwd,
st3r_gs_viewmat_bwd, st3r_gs_render and the fused training calls, st3r_sh_high_adam_step, and render_3dgs at
scene.sh_degree.

References: float64 torch autograd over sh_cases.basis for the stage kernels, under bounds measured per case from a float32
numpy restatement of the chain rule (sh_cases.bounds: 4 x its error, floor 5e-5 of a Gaussian's own gradient); the lower
degree's render for the nesting; the chain of stage calls, bit for bit, for the fused step and for render_3dgs's backward;
float64 torch Adam for the Adam kernel; a fresh context for the history rule.  Run on the MI355X box:
    python -m pytest tests/test_gpu_sh_degree.py -m gpu -q -s
"""
import contextlib
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sh_cases as sc
from per_view_cases import B1, B2, EPS, _same_bits, _setup, dev, make

U = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


@contextlib.contextmanager
def degree(ctx, deg, active=None, v_hi=None):
    from starst3r_amd import ops
    prev = ops.set_sh_degree(ctx, deg, active, v_hi)
    try:
        yield
    finally:
        ops.set_sh_degree(ctx, *prev)


def hi_floats(deg):
    return 3 * (sc.rows(deg) - 4)


def new_hi(N, deg, fill=float("nan")):
    return torch.full((N, hi_floats(deg)), fill, device="cuda:0") if deg >= 2 else None


def sh_grad(g23, v_hi, N, deg):
    """[N, max(K, 4), 3] float64: the sh4 block of grads [23 N] and v_sh_high side by side"""
    a = g23.detach().cpu().numpy().astype(np.float64)[11 * N:].reshape(N, 4, 3)
    if v_hi is None:
        return a
    return np.concatenate([a, v_hi.detach().cpu().numpy().astype(np.float64).reshape(N, -1, 3)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. stage parity
# ---------------------------------------------------------------------------------------------------------------------
_stage = {}


def stage(ctx, N, Cn, deg, active=None):
    """ONE forward, backward and pose backward per (N, Cn, degree, active), shared by the tests and not modified"""
    key = (N, Cn, deg, active)
    if key in _stage:
        return _stage[key]
    from starst3r_amd import ops
    ref = sc.reference(N, Cn, deg if active is None else active)
    case = ref["case"]
    T = dict(means=dev(case.means), quats=dev(case.quats), scales=dev(case.scales), opacities=dev(case.opacities),
             sh=dev(case.sh), vm=dev(case.viewmats), K=dev(case.Ks), campos=dev(sc.campos_of(case.viewmats)))
    v_hi = new_hi(N, deg)
    grads = torch.full((23 * N,), float("nan"), device="cuda:0")
    with degree(ctx, deg, active, v_hi):
        splats, tiles = ops.project_sh(ctx, T["means"], T["quats"], T["scales"], T["opacities"], T["sh"], T["vm"], T["K"],
                                       T["campos"], case.W, case.H, **case.kw)
        ops.project_sh_bwd(ctx, T["means"], T["quats"], T["scales"], T["opacities"], T["sh"], T["vm"], T["K"], T["campos"],
                           case.W, case.H, splats, dev(ref["v"]), eps2d=case.kw["eps2d"], out=grads)
        v_vm = ops.viewmat_bwd(ctx, T["means"], T["quats"], T["scales"], T["sh"], T["vm"], T["K"], T["campos"], case.W,
                               case.H, splats, dev(ref["v"]), eps2d=case.kw["eps2d"])
    torch.cuda.synchronize()
    _stage[key] = dict(ref=ref, splats=splats.cpu().numpy(), grads=grads, v_hi=v_hi, v_vm=v_vm.cpu().numpy())
    return _stage[key]


CASES = [(N, Cn, deg) for N in sc.NS for Cn in sc.CS for deg in sc.DEGREES]


@pytest.mark.parametrize("N,Cn,deg", CASES)
def test_colours_vs_fp64(ctx, N, Cn, deg):
    S = stage(ctx, N, Cn, deg)
    case, r64 = S["ref"]["case"], S["ref"]["r64"]
    sp = S["splats"].reshape(Cn, N, 12)
    assert np.array_equal(sp[..., 10].view(np.int32) > 0, case.vis)
    col, want = sp[..., 6:9][case.vis], r64["colour"][case.vis]
    np.testing.assert_allclose(col, want, rtol=1e-5, atol=1e-6)
    assert np.array_equal(col == 0, want == 0)              # every |pre-clamp| >= 1e-3: the same channels are clamped


@pytest.mark.parametrize("N,Cn,deg", CASES)
def test_backward_vs_fp64_autograd(ctx, N, Cn, deg):
    """cotangents on the colour columns only: sh4 + v_sh_high are the coefficient gradients, the means block is the
    direction term alone, everything else of grads is zero (no regulariser)"""
    S = stage(ctx, N, Cn, deg)
    r64, bnd = S["ref"]["r64"], S["ref"]["bounds"]
    K = sc.rows(deg)
    got = sh_grad(S["grads"], S["v_hi"], N, deg)
    assert np.isfinite(got).all()                            # NaN cotangents of culled pairs never read, v_sh_high whole
    assert not got[:, K:].any()                              # degree 0: rows 1..3 of the sh4 block are zeros
    g = S["grads"].cpu().numpy().astype(np.float64)
    x_sh = sc.excess(got[:, :K], r64, bnd, "sh")
    x_m = sc.excess(g[:3 * N].reshape(N, 3), r64, bnd, "means")
    print("n%d c%d deg%d: error / bound sh %.3f (rel %.1e) means %.3f (rel %.1e)"
          % (N, Cn, deg, x_sh, bnd["sh"]["rel"], x_m, bnd["means"]["rel"]))
    assert x_sh <= 1.0 and x_m <= 1.0
    assert not g[3 * N:11 * N].any()


@pytest.mark.parametrize("N,Cn,deg", CASES)
def test_viewmat_bwd_vs_fp64_autograd(ctx, N, Cn, deg):
    S = stage(ctx, N, Cn, deg)
    r64, bnd = S["ref"]["r64"], S["ref"]["bounds"]
    x = sc.excess(S["v_vm"], r64, bnd, "viewmats")
    print("n%d c%d deg%d: error / bound viewmats %.3f (rel %.1e)" % (N, Cn, deg, x, bnd["viewmats"]["rel"]))
    assert x <= 1.0
    if deg == 0:
        assert not S["v_vm"].any()                           # no view dependence at all


@pytest.mark.parametrize("deg,active", [(3, 0), (3, 1), (3, 2), (2, 0), (2, 1)])
def test_active_below_degree_zeroes_the_higher_bands(ctx, deg, active):
    """(degree, active): the colours, sh4 and pose gradient of degree `active`, bit for bit; v_sh_high written whole, its
    rows of the bands in use those of (active, active), the rest zeros"""
    N, Cn = 257, 2
    A, B = stage(ctx, N, Cn, deg, active), stage(ctx, N, Cn, active)
    assert np.array_equal(A["splats"].view(np.uint32), B["splats"].view(np.uint32))
    assert _same_bits(A["grads"], B["grads"])
    assert np.array_equal(A["v_vm"].view(np.uint32), B["v_vm"].view(np.uint32))
    hi = A["v_hi"].cpu().numpy()
    used = hi_floats(active) if active >= 2 else 0
    assert not hi[:, used:].view(np.uint32).any()
    if used:
        assert np.array_equal(hi[:, :used].view(np.uint32), B["v_hi"].cpu().numpy().view(np.uint32))
        assert hi[:, :used].any()


def test_backward_without_v_sh_high_is_invalid_and_forward_is_not(ctx):
    from starst3r_amd import _lib, ops
    S = stage(ctx, 257, 2, 3)
    case = S["ref"]["case"]
    T = [dev(a) for a in (case.means, case.quats, case.scales, case.opacities, case.sh, case.viewmats, case.Ks,
                          sc.campos_of(case.viewmats))]
    with degree(ctx, 3):
        splats, _ = ops.project_sh(ctx, *T, case.W, case.H, **case.kw)
        assert np.array_equal(splats.cpu().numpy().view(np.uint32), S["splats"].view(np.uint32))
        with pytest.raises(ValueError, match="v_sh_high"):   # ST3R_ERR_INVALID (_lib.check)
            ops.project_sh_bwd(ctx, *T, case.W, case.H, splats, dev(S["ref"]["v"]))
        with pytest.raises(ValueError, match="sh_stride"):   # 4 rows are not 16
            ops.project_sh(ctx, *T[:4], T[4][:, :4].contiguous(), *T[5:], case.W, case.H, **case.kw)
    for bad in ((4, 4), (2, 3), (-1, -1)):
        assert _lib.lib().st3r_ctx_set_sh_degree(ctx.handle, bad[0], bad[1], None) != 0
    assert _lib.lib().st3r_ctx_set_sh_degree(ctx.handle, 1, 1, T[0].data_ptr()) != 0   # v_sh_high with degree <= 1
    assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT


# ---------------------------------------------------------------------------------------------------------------------
# 2. nesting: zero rows above a degree render with that degree's bits
# ---------------------------------------------------------------------------------------------------------------------
def _scene(ctx, name="small", sh_seed=11, sh_amp=0.25):
    """per_view_cases' scene with view-dependent colour in all 16 rows -> P, vm, K, campos, W, H"""
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    P = {k: dev(v) for k, v in g.items()}
    gen = torch.Generator().manual_seed(sh_seed)
    P["shN"][:, 1:16] = (sh_amp * (2 * torch.rand((P["shN"].shape[0], 15, 3), generator=gen) - 1)).cuda()
    vm, K = dev(w2c), dev(Ks)
    return P, vm, K, ops.camera_positions(vm), W, H


@pytest.mark.parametrize("hi,lo", [(2, 1), (3, 1), (3, 2), (1, 0)])
def test_render_nests(ctx, hi, lo):
    from starst3r_amd import ops
    P, vm, K, campos, W, H = _scene(ctx)
    P["shN"][:, sc.rows(lo):] = 0
    with degree(ctx, hi):
        a, aa, _ = ops.render(ctx, P, vm, K, campos, W, H)
    with degree(ctx, lo):
        b, ba, _ = ops.render(ctx, P, vm, K, campos, W, H)
    torch.cuda.synchronize()
    assert float(a.abs().max()) > 0
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(aa.cpu().numpy(), ba.cpu().numpy())
    if lo == 1:   # the default setting is the same kernel
        c, _, _ = ops.render(ctx, P, vm, K, campos, W, H)
        assert _same_bits(c, b)


def test_render_degrees_differ(ctx):
    from starst3r_amd import ops
    P, vm, K, campos, W, H = _scene(ctx)
    out = []
    for d in sc.DEGREES:
        with degree(ctx, d):
            out.append(ops.render(ctx, P, vm, K, campos, W, H)[0].clone())
    for d in (1, 2, 3):
        assert float((out[d] - out[d - 1]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fused step at degree 3 is the chain of stage calls
# ---------------------------------------------------------------------------------------------------------------------
def _unfused_step(ctx, P, vm, K, gt, W, H, deg, active, v_hi, ssim_fac, want_pose):
    from starst3r_amd import ops
    Cn = vm.shape[0]
    with degree(ctx, deg, active, v_hi):
        rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
        _, v_y = ops.loss_l1_ssim(ctx, rgb, gt, 1.0 - ssim_fac, ssim_fac, want_grad=True)
        v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                                 info["_last_ids"], v_y, None, info["_cum_tiles"], Cn, W, H)
        grads = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K,
                                   info["_campos"], W, H, info["_splats"], v_splats)
        v_vm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H,
                               info["_splats"], v_splats) if want_pose else None
    return grads, v_vm


@pytest.mark.parametrize("name,deg,active,poses", [("small", 3, 3, False), ("ragged", 3, 3, True), ("many", 2, 2, False),
                                                   ("small", 3, 1, True), ("small", 0, 0, False)])
def test_fused_step_equals_stage_chain(name, deg, active, poses):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P, vm, K, campos, W, H = _scene(ctx, name)
    with degree(ctx, 3):
        gt = ops.render(ctx, P, vm, K, campos, W, H)[0].clone()
    gt = torch.clamp(gt + 0.05 * torch.randn(gt.shape, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1)),
                     0, 1).contiguous()
    N, Cn = P["means"].shape[0], vm.shape[0]
    lr, step = 1e-3, 3
    mom = lambda n, s: 1e-3 * torch.randn(n, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(s))
    m0, v0 = mom(23 * N, 2), mom(23 * N, 3).abs()
    # unfused
    Pu = {k: v.clone() for k, v in P.items()}
    hi_u = new_hi(N, deg)
    g_u, vvm_u = _unfused_step(ctx, Pu, vm, K, gt, W, H, deg, active, hi_u, 0.2, poses)
    m_u, v_u = m0.clone(), v0.clone()
    ops.adam_step(ctx, Pu, g_u, m_u, v_u, lr, B1, B2, EPS, step)
    if deg >= 2:
        hm_u, hv_u = mom(N * hi_floats(deg), 4).view(N, -1), mom(N * hi_floats(deg), 5).abs().view(N, -1)
        ops.sh_high_adam_step(ctx, Pu["shN"], deg, hi_u, hm_u, hv_u, lr, B1, B2, EPS, step)
    # fused
    Pf = {k: v.clone() for k, v in P.items()}
    hi_f = new_hi(N, deg)
    g_f = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    m_f, v_f = m0.clone(), v0.clone()
    with degree(ctx, deg, active, hi_f):
        if poses:
            vvm_f = torch.full((Cn, 4, 4), 7.0, device="cuda:0")
            vm_f, cp_f = vm.clone(), campos.clone()
            ops.train_step_poses(ctx, Pf, vm_f, K, cp_f, gt, W, H, 0.2, 0.0, 0.0, g_f, m_f, v_f, lr, B1, B2, EPS, step, loss,
                                 torch.zeros(6 * Cn, device="cuda:0"), torch.zeros(6 * Cn, device="cuda:0"), 0.0, 1,
                                 v_viewmats_out=vvm_f)
        else:
            ops.train_step(ctx, Pf, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, g_f, m_f, v_f, lr, B1, B2, EPS, step, loss)
    if deg >= 2:
        hm_f, hv_f = mom(N * hi_floats(deg), 4).view(N, -1), mom(N * hi_floats(deg), 5).abs().view(N, -1)
        ops.sh_high_adam_step(ctx, Pf["shN"], deg, hi_f, hm_f, hv_f, lr, B1, B2, EPS, step)
    torch.cuda.synchronize()
    assert _same_bits(g_f, g_u)
    assert _same_bits(m_f, m_u) and _same_bits(v_f, v_u)
    for k in P:
        assert _same_bits(Pf[k], Pu[k]), k
    if deg >= 2:
        assert _same_bits(hi_f, hi_u) and _same_bits(hm_f, hm_u) and _same_bits(hv_f, hv_u)
        assert bool(torch.isfinite(hi_f).all())
        if active >= 2:
            assert float(hi_f.abs().max()) > 0 and not _same_bits(Pf["shN"][:, 4:sc.rows(active)], P["shN"][:, 4:sc.rows(active)])
        assert _same_bits(Pf["shN"][:, sc.rows(deg):], P["shN"][:, sc.rows(deg):])   # rows nobody trains
    if poses:
        assert _same_bits(vvm_f, vvm_u)
    ctx.close()


@pytest.mark.parametrize("deg,active", [(3, 3), (3, 2)])
def test_fused_step_with_the_activation_on_equals_the_chain(deg, active):
    """log-scales and logits under st3r_ctx_set_activation at degree 3: grads and v_sh_high of st3r_gs_train_fwd_bwd are
    those of st3r_param_activate -> the stage chain on the activated copies -> st3r_param_activate_bwd, bit for bit"""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P, vm, K, campos, W, H = _scene(ctx, "small")
    with degree(ctx, 3):
        gt = (0.9 * ops.render(ctx, P, vm, K, campos, W, H)[0]).contiguous()
    P["scales"] = torch.log(P["scales"].abs().clamp(min=1e-4)).contiguous()
    o = P["opacities"].clamp(0.05, 0.95)
    P["opacities"] = torch.log(o / (1 - o)).contiguous()
    N = P["means"].shape[0]
    # the chain
    S, O, _ = ops.param_activate(ctx, P["scales"], P["opacities"], want_sums=True)
    PA = dict(P, scales=S, opacities=O)
    hi_u = new_hi(N, deg)
    g_u, _ = _unfused_step(ctx, PA, vm, K, gt, W, H, deg, active, hi_u, 0.2, False)
    G = ops.split_grads(g_u, N)
    ops.param_activate_bwd(ctx, S, O, G["scales"], G["opacities"], 0.0, 0.0, G["scales"], G["opacities"])
    # fused
    hi_f = new_hi(N, deg)
    g_f = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    ops.set_activation(ctx, True)
    try:
        with degree(ctx, deg, active, hi_f):
            ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, g_f, loss)
    finally:
        ops.set_activation(ctx, False)
    torch.cuda.synchronize()
    assert _same_bits(g_f, g_u) and _same_bits(hi_f, hi_u)
    assert float(hi_f[:, :hi_floats(active)].abs().max()) > 0 and float(g_f[7 * N:11 * N].abs().max()) > 0
    ctx.close()


def test_view_chunks_add_up_in_v_sh_high():
    """debug flag 32: nine views in chunks of four and five; the later chunk ADDS to grads and to v_sh_high (preset to
    NaN: the first chunk must overwrite).  The sums are those of the whole call in another order: the agreement
    test_gpu_exposure asks of the Gaussian gradients of a chunked call (1e-6 of the largest entry)."""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P, vm, K, campos, W, H = _scene(ctx, "many")
    with degree(ctx, 3):
        gt = ops.render(ctx, P, vm, K, campos, W, H)[0].clone()
    gt = (0.9 * gt).contiguous()
    N = P["means"].shape[0]
    out = []
    for flags in (0, 32):
        hi = new_hi(N, 3)
        g = torch.full((23 * N,), float("nan"), device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
        ops.set_debug(ctx, flags)
        try:
            with degree(ctx, 3, 3, hi):
                ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, g, loss)
        finally:
            ops.set_debug(ctx, 0)
        torch.cuda.synchronize()
        out.append((g, hi))
    (g0, h0), (g1, h1) = out
    assert bool(torch.isfinite(h1).all()) and float(h0.abs().max()) > 0
    assert float((h1 - h0).abs().max() / h0.abs().max()) < 1e-6
    assert float((g1 - g0).abs().max() / g0.abs().max()) < 1e-6
    ctx.close()


def test_sh_degree_with_a_communicator_is_invalid():
    from starst3r_amd import dist as sdist, ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    N = P["means"].shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    hi = new_hi(N, 3, 7.0)
    loss = torch.zeros(1, device="cuda:0")
    before = [x.clone() for x in list(P.values()) + [grads, m, v, hi]]
    sdist.attach_native_comm(ctx)
    try:
        for setting in ((3, 3, hi), (0, 0, None), (1, 0, None)):
            with degree(ctx, *setting):
                with pytest.raises(ValueError, match="communicator"):
                    ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, loss)
        # (once: the next exchanged step would report this one's failure, as the protocol of comm.hip has it)
        with degree(ctx, 3, 3, hi):
            with pytest.raises(ValueError, match="communicator"):
                ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, 1, loss)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(list(P.values()) + [grads, m, v, hi], before))
    finally:
        sdist.detach_native_comm(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Adam on the high block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,deg,rows_total", [(1, 2, 9), (257, 3, 16), (1000, 3, 24), (255, 2, 24)])
def test_sh_high_adam_vs_fp64(ctx, N, deg, rows_total):
    """three steps against torch's Adam formulas in float64 on the same float32 inputs.  Bound per scalar and step: the
    kernel's float32 arithmetic rounds m, v, sqrt, two quotients, a product and the difference -- 8 roundings of quantities
    whose effect on the update is at most the update's own size lr (|mhat| / (sqrt(vhat) + eps) <= 1 up to the bias
    corrections' ratio, <= 1 / (1 - B1) at step 1 scaled back by 1 - B1), plus one rounding of the parameter: 8 U lr per
    step on the update, U |p| on the stored value; moments 4 U per step of the sum of their terms' magnitudes (m's terms
    change sign from step to step)."""
    from starst3r_amd import ops
    gen = torch.Generator().manual_seed(100 + N)
    Hn = hi_floats(deg)
    sh0 = torch.randn((N, rows_total, 3), generator=gen)
    lr, steps = 1e-2, 3
    sh = sh0.clone().cuda()
    m = torch.zeros((N, Hn), device="cuda:0"); v = torch.zeros_like(m)
    p64 = sh0[:, 4:sc.rows(deg)].reshape(N, Hn).double().clone()
    m64, v64, mabs = torch.zeros_like(p64), torch.zeros_like(p64), torch.zeros_like(p64)
    for t in range(1, steps + 1):
        g = torch.randn((N, Hn), generator=gen) * (10.0 ** torch.randint(-4, 1, (N, Hn), generator=gen).float())
        ops.sh_high_adam_step(ctx, sh, deg, g.cuda(), m, v, lr, B1, B2, EPS, t)
        g64 = g.double()
        m64 = B1 * m64 + (1 - B1) * g64
        mabs = B1 * mabs + (1 - B1) * g64.abs()
        v64 = B2 * v64 + (1 - B2) * g64 * g64
        p64 = p64 - lr * (m64 / (1 - B1 ** t)) / ((v64 / (1 - B2 ** t)).sqrt() + EPS)
    torch.cuda.synchronize()
    got = sh.cpu()
    err = (got[:, 4:sc.rows(deg)].reshape(N, Hn).double() - p64).abs()
    bound = steps * (8 * U * lr + U * p64.abs().clamp(min=1.0))
    print("sh_high_adam n%d deg%d: worst error / bound %.3f" % (N, deg, float((err / bound).max())))
    assert bool((err <= bound).all())
    assert bool(((m.cpu().double() - m64).abs() <= 4 * steps * U * mabs + 1e-30).all())
    assert bool(((v.cpu().double() - v64).abs() <= 4 * steps * U * v64.abs() + 1e-30).all())
    # rows 0..3 and the rows above the degree keep their bits
    assert torch.equal(got[:, :4], sh0[:, :4]) and torch.equal(got[:, sc.rows(deg):], sh0[:, sc.rows(deg):])


def test_overflowing_async_step_moves_no_high_coefficient():
    """debug flag 8 halves the capacity of an asynchronous step (test_gpu_exposure's way): its Adam updates are skipped on
    the device -- the high block's too --, st3r_ctx_settle reports it, and the repeated step gives the undisturbed run"""
    from per_view_cases import _medium
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        ctx = ops.Context("cuda:0")
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        P = {k: v.clone() for k, v in P0.items()}
        gen = torch.Generator().manual_seed(5)
        P["shN"][:, 4:16] = (0.1 * torch.randn((P["shN"].shape[0], 12, 3), generator=gen)).cuda()
        N = P["means"].shape[0]
        grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
        hi = new_hi(N, 3, 0.0); hm = torch.zeros_like(hi); hv = torch.zeros_like(hi)
        losses = torch.zeros(3, device="cuda:0")
        state = lambda: [P[k] for k in sorted(P)] + [m, v, hm, hv]
        it = 0
        with degree(ctx, 3, 3, hi):
            while it < 3:
                before = [x.clone() for x in state()] if it == overflow_at else None
                if it == overflow_at:
                    ops.set_debug(ctx, 8)
                ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, it + 1,
                               losses[it:it + 1], want_stats=False)
                ops.sh_high_adam_step(ctx, P["shN"], 3, hi, hm, hv, 1e-3, B1, B2, EPS, it + 1)
                ops.set_debug(ctx, 0)
                if it == overflow_at:
                    overflow_at = -1
                    with pytest.raises(_lib.St3rError) as e:
                        ops.settle(ctx)
                    assert e.value.code == -3
                    for x, y in zip(state(), before):
                        assert _same_bits(x, y)
                    continue
                it += 1
            ops.settle(ctx)
        torch.cuda.synchronize()
        ctx.close()
        return state()
    a, b = steps(-1), steps(1)
    assert float(a[-2].abs().max()) > 0
    for x, y in zip(a, b):
        assert _same_bits(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 5. history: a set-and-restored setting leaves a context whose next call gives a fresh context's bits
# ---------------------------------------------------------------------------------------------------------------------
def test_restored_default_gives_a_fresh_contexts_bits():
    from starst3r_amd import ops

    def default_step(ctx, P0, vm, K, campos, gt, W, H):
        P = {k: v.clone() for k, v in P0.items()}
        N = P["means"].shape[0]
        g = torch.full((23 * N,), 7.0, device="cuda:0"); m = torch.zeros_like(g); v = torch.zeros_like(g)
        loss = torch.zeros(1, device="cuda:0")
        # (render first: every call of this test then sees the same Gaussians, and the grow-only arena the same counts)
        rgb = ops.render(ctx, P, vm, K, campos, W, H)[0].clone()
        stats = ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, g, m, v, 1e-3, B1, B2, EPS, 1, loss)
        torch.cuda.synchronize()
        return [P[k] for k in sorted(P)] + [g, m, v, loss, rgb], stats, ctx.arena_bytes()

    fresh = ops.Context("cuda:0")
    P0, vm, K, campos, W, H = _scene(fresh)
    gt = (0.9 * ops.render(fresh, P0, vm, K, campos, W, H)[0]).contiguous()
    fresh.close()
    fresh = ops.Context("cuda:0")
    want, want_stats, want_arena = default_step(fresh, P0, vm, K, campos, gt, W, H)
    fresh.close()
    used = ops.Context("cuda:0")
    N = P0["means"].shape[0]
    hi = new_hi(N, 3)
    P = {k: v.clone() for k, v in P0.items()}
    g = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(g); v = torch.zeros_like(g)
    with degree(used, 3, 2, hi):
        ops.render(used, P, vm, K, campos, W, H)
        ops.train_step(used, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, g, m, v, 1e-3, B1, B2, EPS, 1,
                       torch.zeros(1, device="cuda:0"))
    assert ops.get_sh_degree(used) == ops.SH_DEFAULT
    got, got_stats, got_arena = default_step(used, P0, vm, K, campos, gt, W, H)
    used.close()
    for x, y in zip(got, want):
        assert _same_bits(x, y)
    assert got_stats == want_stats and got_arena == want_arena


# ---------------------------------------------------------------------------------------------------------------------
# 6. render_3dgs at scene.sh_degree
# ---------------------------------------------------------------------------------------------------------------------
def _api_scene(ctx, deg):
    P, vm, K, campos, W, H = _scene(ctx)
    scene = types.SimpleNamespace(device=torch.device("cuda:0"), gaussians={k: torch.nn.Parameter(v.clone()) for k, v in P.items()})
    if deg != "absent":
        scene.sh_degree = deg
    return scene, P, vm, K, W, H


@pytest.mark.parametrize("deg", [0, 2, 3])
def test_render_3dgs_backward_is_the_stage_chain_at_the_scenes_degree(ctx, deg):
    """render_3dgs back-propagated into shN and w2c equals the chain of stage calls under the setting, bit for bit -- and
    that chain is held against float64 autograd by the stage tests above; the setting is restored behind each half"""
    from starst3r_amd import gs, ops
    scene, P, vm, K, W, H = _api_scene(ctx, deg)
    w2c = vm.clone().requires_grad_()
    img, alpha, info = gs.render_3dgs(scene, w2c, K, W, H)
    assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT
    with degree(ctx, deg):
        want = ops.render(ctx, P, vm, K, ops.camera_positions(vm), W, H)[0]
    assert _same_bits(img.detach(), want)
    gen = torch.Generator("cuda:0").manual_seed(8)
    v_img = torch.randn(img.shape, device="cuda:0", generator=gen)
    (img * v_img).sum().backward()
    assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT
    N, Cn = P["means"].shape[0], vm.shape[0]
    hi = new_hi(N, deg)
    with degree(ctx, deg, deg, hi):
        rgb, al, inf = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
        v_splats = ops.blend_bwd(ctx, inf["_splats"], inf["isect_offsets"], inf["_flatten_ids_dense"], al, inf["_last_ids"],
                                 v_img.contiguous(), None, inf["_cum_tiles"], Cn, W, H)
        g = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, inf["_campos"], W, H,
                               inf["_splats"], v_splats)
        v_vm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, inf["_campos"], W, H,
                               inf["_splats"], v_splats)
    v_sh = scene.gaussians["shN"].grad
    Kr = sc.rows(deg)
    assert _same_bits(v_sh[:, :4].reshape(-1), g[11 * N:])
    if deg >= 2:
        assert _same_bits(v_sh[:, 4:Kr].reshape(N, -1), hi) and float(hi.abs().max()) > 0
    assert not bool(v_sh[:, max(Kr, 4):].any())
    assert _same_bits(w2c.grad, v_vm)
    assert _same_bits(scene.gaussians["means"].grad.reshape(-1), g[:3 * N])


@pytest.mark.parametrize("name", ["small", "many"])
def test_render_3dgs_grads_at_degree_2_vs_dense_fp64(ctx, name, monkeypatch):
    """render_3dgs at scene.sh_degree = 2 back-propagated into shN and w2c against float64 autograd through
    oracle.gs_torch_ref's dense renderer with sh_cases.basis for the colours (test_gpu_pose_grad's end-to-end check and its
    bar, 5e-5 of a camera's largest entry; the same bar for shN, of the tensor's largest entry: both sum the same
    per-pair float32 terms)"""
    import starst3r_amd as st
    from oracle import gs_torch_ref as tr
    from per_view_cases import masked_cotangents, rel_err_per_camera
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    g = dict(g)
    rng = np.random.default_rng(3)
    sh = g["shN"].copy(); sh[:, 1:9] = rng.uniform(-0.25, 0.25, sh[:, 1:9].shape)
    sh[:, 9:] = 0.0
    g["shN"] = sh.astype(np.float32)
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H, seed=11)
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    scene.sh_degree = 2
    w = dev(w2c).requires_grad_()
    rgb, alpha, _ = scene.render_3dgs(w, dev(Ks), W, H)
    ((rgb * dev(v_rgb)).sum() + (alpha * dev(v_alpha)).sum()).backward()
    info = ops.last_info()
    N, Cn = g["means"].shape[0], w2c.shape[0]
    rad = info["_splats"][:, 10].view(torch.int32).reshape(Cn, N).cpu().to(torch.int64)

    def sh_color2(means, campos, k):
        d = means - campos
        d = d / d.norm(dim=-1, keepdim=True)
        b = torch.stack(sc.basis(d[:, 0], d[:, 1], d[:, 2], 2), 1)            # [n, 9]
        return torch.clamp_min(torch.einsum("nk,nkj->nj", b, k[:, :9]) + 0.5, 0.0)
    monkeypatch.setattr(tr, "sh_color", sh_color2)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    vm, k64 = t(w2c).requires_grad_(), t(g["shN"]).requires_grad_()
    rgb_t, alpha_t = tr.render_dense(t(g["means"]), t(g["quats"]), t(g["scales"]), t(g["opacities"]), k64, vm, t(Ks), W, H,
                                     rad > 0, rad)
    ((rgb_t * t(v_rgb)).sum() + (alpha_t * t(v_alpha)).sum()).backward()
    err = rel_err_per_camera(w.grad, vm.grad)
    v_sh = scene.gaussians["shN"].grad.double().cpu()
    e_sh = float((v_sh - k64.grad).abs().max() / k64.grad.abs().max())
    print(name, "degree 2 end to end: w2c max |d| / max |ref| per camera", ["%.1e" % e for e in err], "shN %.1e" % e_sh)
    assert float(k64.grad[:, 4:9].abs().max()) > 0 and not bool(v_sh[:, 9:].any())
    assert max(err) <= 5e-5 and e_sh <= 5e-5


def test_sh_degree_none_is_a_scene_without_the_attribute(ctx):
    from starst3r_amd import gs
    outs = []
    for deg in ("absent", None):
        scene, P, vm, K, W, H = _api_scene(ctx, deg)
        w2c = vm.clone().requires_grad_()
        img, alpha, _ = gs.render_3dgs(scene, w2c, K, W, H)
        (img.sum() + alpha.sum()).backward()
        outs.append([img.detach(), alpha.detach(), w2c.grad] + [scene.gaussians[k].grad for k in sorted(scene.gaussians)])
    for x, y in zip(*outs):
        assert (x is None and y is None) or _same_bits(x, y)


def _grey_scene(**settings):
    """per_view_cases' small scene against mid-grey photographs, with the given settings of the scene"""
    from per_view_cases import _optim_scene
    g, w2c, Ks, W, H = make("small")
    imgs = np.full((w2c.shape[0], H, W, 3), 0.5, np.float32)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
    for k, v in settings.items():
        setattr(scene, k, v)
    return scene


def test_run_3dgs_optim_schedule_and_persistence(ctx):
    """sh_degree 3, one more band every 2 steps: the rows 4..8 first move at step 5 (counter 5: degree 2), the rows 9..15 at
    step 7; the rows 16.. never; a second call continues counter and moments; the setting is the call's"""
    from starst3r_amd import ops
    scene = _grey_scene(sh_degree=3, sh_degree_interval=2)
    sh0 = scene.gaussians["shN"].data.clone()
    moved = lambda a, b: not _same_bits(scene.gaussians["shN"].data[:, a:b], sh0[:, a:b])
    seen = []
    for it in range(1, 8):
        losses = scene.run_3dgs_optim(1)
        assert len(losses) == 1 and np.isfinite(losses[0])
        seen.append((moved(1, 4), moved(4, 9), moved(9, 16)))
        assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT
    #          t = 1, 2 (degree 0)                      3, 4 (degree 1)      5, 6 (degree 2)   7 (degree 3)
    assert seen == [(False, False, False)] * 2 + [(True, False, False)] * 2 + [(True, True, False)] * 2 + [(True, True, True)]
    assert not moved(16, 24)
    st = scene._gs_optim
    N = sh0.shape[0]
    assert st.step == 7 and st.sh_step == 7 and tuple(st.sh_m.shape) == (N, 36) and tuple(st.sh_v.shape) == (N, 36)
    m_before, obj = st.sh_m.clone(), st.sh_m
    scene.run_3dgs_optim(2)
    assert st.sh_step == 9 and st.sh_m is obj and not _same_bits(st.sh_m, m_before)
    # together with other options; refused with the refinement at degree >= 2, before anything runs
    both = scene.run_3dgs_optim(2, pose_lr=1e-5, exposure_lr=1e-4)
    assert len(both) == 2 and all(np.isfinite(both)) and st.sh_step == 11
    class Foreign(type(scene.strategy)):
        pass
    own = scene.strategy
    scene.strategy = Foreign()
    with pytest.raises(NotImplementedError, match="sh_degree"):      # another strategy object, before anything runs
        scene.run_3dgs_optim(1, enable_pruning=True)
    scene.strategy = own
    assert st.step == 11
    # the full degree from the first step without an interval; sh_high_lr 0 leaves the high rows alone
    full = _grey_scene(sh_degree=2)
    sh0 = full.gaussians["shN"].data.clone()
    full.run_3dgs_optim(1)
    assert not _same_bits(full.gaussians["shN"].data[:, 4:9], sh0[:, 4:9])
    assert _same_bits(full.gaussians["shN"].data[:, 9:], sh0[:, 9:])
    still = _grey_scene(sh_degree=2, sh_high_lr=0.0)
    still.run_3dgs_optim(2)
    assert _same_bits(still.gaussians["shN"].data[:, 4:], sh0[:, 4:]) and float(still._gs_optim.sh_m.abs().max()) > 0


def test_refine_step_resets_the_sources_high_moments_and_grows_them(ctx):
    """enable_pruning at degree 3 under the project's own MCMCStrategy, one refinement step (the window moved onto
    iteration 2): the Gaussians the relocation drew as sources (st3r_ctx_peek 7) have zero rows in sh_m / sh_v, every
    other old row keeps the bits it had in front of the hook, and sh_m, sh_v, sh_grad grow with zeros with the set"""
    from starst3r_amd import ops
    scene = _grey_scene(sh_degree=3)
    scene.strategy.refine_start_iter, scene.strategy.refine_every = 1, 2          # is_refine_step(2) only, in four steps
    N = scene.gaussians["means"].shape[0]
    scene.gaussians["opacities"].data[::7] = -20.0                                 # dead for the relocation: logit -20
    seen = {}
    post = scene.strategy.step_post_backward

    def watching(params, optimizers, state, step, info, lr):
        st = scene._gs_optim
        if scene.strategy.is_refine_step(step):
            seen["m"], seen["v"] = st.sh_m.clone(), st.sh_v.clone()
        post(params, optimizers, state, step, info, lr)
        if scene.strategy.is_refine_step(step):
            seen["after"] = (st.sh_m.clone(), st.sh_v.clone(), st.sh_grad.clone(), state["n_relocated"], state["n_added"])
    scene.strategy.step_post_backward = watching
    # the draw counts are overwritten by the growth that follows the relocation: read them between the two
    relocate = ops.mcmc_relocate

    def relocate_and_keep(c, P, m, v, min_opacity, seed, call, want_count=True):
        n = relocate(c, P, m, v, min_opacity, seed, call, want_count)
        seen["src"] = (ops.peek(c, 7, N, torch.int32) > 0).clone()
        return n
    ops.mcmc_relocate = relocate_and_keep
    try:
        losses = scene.run_3dgs_optim(4, enable_pruning=True)
    finally:
        ops.mcmc_relocate = relocate
        del scene.strategy.step_post_backward
    assert len(losses) == 4 and all(np.isfinite(losses))
    m1, v1, g1, n_rel, n_add = seen["after"]
    src = seen["src"]
    assert n_rel > 0 and n_add > 0 and 0 < int(src.sum()) < N
    assert float(seen["m"].abs().max()) > 0 and float(seen["m"][src].abs().max()) > 0
    assert not bool(m1[:N][src].any()) and not bool(v1[:N][src].any())
    assert _same_bits(m1[:N][~src], seen["m"][~src]) and _same_bits(v1[:N][~src], seen["v"][~src])
    assert tuple(m1.shape) == tuple(v1.shape) == tuple(g1.shape) == (N + n_add, 36)
    assert not bool(m1[N:].any()) and not bool(v1[N:].any())
    st = scene._gs_optim
    assert scene.gaussians["shN"].shape[0] == N + n_add == st.sh_m.shape[0] and st.sh_step == 4
    # the step behind it trained on the grown tensors (the new Gaussians themselves carry the logits the raw renderer reads
    # as opacities, SURVEY App. B-1: whether they are visible is the reference's quirk, not this test's subject)
    assert not _same_bits(st.sh_m[:N], m1[:N]) and bool(torch.isfinite(st.sh_m).all())


def test_run_3dgs_optim_with_sh_degree_none_is_a_scene_without_it(ctx):
    outs = []
    for settings in ({}, dict(sh_degree=None, sh_degree_interval=5, sh_high_lr=1.0)):
        scene = _grey_scene(**settings)
        losses = scene.run_3dgs_optim(4)
        st = scene._gs_optim
        assert not hasattr(st, "sh_m") and not hasattr(st, "sh_step")
        outs.append([torch.tensor(losses), st.m, st.v] + [scene.gaussians[k].data for k in sorted(scene.gaussians)])
    for x, y in zip(*outs):
        assert _same_bits(x, y)


def test_init_3dgs_canonical_under_the_setting(ctx):
    import starst3r_amd as st3r
    from starst3r_amd import gs
    pts = torch.rand(50, 3); cols = torch.rand(50, 3)
    out = {}
    for deg in ("absent", None, 3):
        scene = st3r.Scene(device="cuda:0")
        scene.dense_pts, scene.dense_cols = [pts[:20], pts[20:]], [cols[:20], cols[20:]]
        if deg != "absent":
            scene.sh_degree = deg
        gs.init_3dgs(scene)
        out[deg] = {k: v.data.cpu() for k, v in scene.gaussians.items()}
    for k in out["absent"]:
        assert torch.equal(out["absent"][k], out[None][k])
    assert torch.equal(out["absent"]["shN"], (1 - cols)[:, None, :].expand(50, 24, 3))       # the reference's
    dc = (cols - 0.5) / 0.2820947917738781
    assert torch.equal(out[3]["shN"][:, 0], dc) and torch.equal(out[3]["sh0"][:, 0], dc)
    assert not out[3]["shN"][:, 1:].any()
    for k in ("means", "scales", "quats", "opacities"):
        assert torch.equal(out[3][k], out["absent"][k])


# ---------------------------------------------------------------------------------------------------------------------
# 7. purpose: degree 3 explains view-dependent colour that degree 1 cannot
# ---------------------------------------------------------------------------------------------------------------------
def test_degree_3_reaches_a_lower_loss_than_degree_1_on_degree_3_colour():
    """about 2 000 Gaussians with degree-3 ground-truth colour, rendered by the library itself into four 80 x 48 views;
    trained from the canonical DC-only initialisation for the same number of steps at degree 1 and at degree 3.  The two
    runs are compared with each other, not with a constant."""
    from st3r_synth import synth
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    N, V, W, H, steps = 2000, 4, 80, 48, 150
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=17, scale_lo=0.02, scale_hi=0.08)
    P0 = {k: dev(v) for k, v in g.items()}
    gen = torch.Generator().manual_seed(23)
    truth = P0["shN"].clone()
    truth[:, 1:16] = (0.5 * (2 * torch.rand((N, 15, 3), generator=gen) - 1)).cuda()
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    with degree(ctx, 3):
        gt = ops.render(ctx, dict(P0, shN=truth), vm, K, campos, W, H)[0].clone().contiguous()
    final = {}
    for deg in (1, 3):
        P = {k: v.clone() for k, v in P0.items()}
        P["shN"][:, 1:] = 0                                     # DC only
        grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
        hi = new_hi(N, deg, 0.0)
        hm = torch.zeros_like(hi) if deg >= 2 else None; hv = torch.zeros_like(hi) if deg >= 2 else None
        losses = torch.zeros(steps, device="cuda:0")
        with degree(ctx, deg, deg, hi):
            for it in range(steps):
                ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads, m, v, 2e-3, B1, B2, EPS, it + 1,
                               losses[it:it + 1])
                if deg >= 2:
                    ops.sh_high_adam_step(ctx, P["shN"], deg, hi, hm, hv, 2e-3, B1, B2, EPS, it + 1)
        torch.cuda.synchronize()
        final[deg] = (float(losses[0]), float(losses[-5:].mean()))
    ctx.close()
    print("purpose: loss first -> last five, degree 1 %.5f -> %.5f, degree 3 %.5f -> %.5f" % (final[1] + final[3]))
    assert final[1][0] == final[3][0]                          # the same start: rows 1.. are zero in both
    assert final[3][1] < final[1][1]
