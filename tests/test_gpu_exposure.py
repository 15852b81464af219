"""Per-view exposure: st3r_exposure_fwd / _bwd / _adam_step (gs_exposure.hip), st3r_ctx_set_exposure inside the fused steps
(fused_step.hip), run_3dgs_optim(exposure_lr=..., exposure_freeze=...) and render_3dgs(exposure=...).

References: float64 torch autograd for the stage kernels; the update rule restated in float64 torch for the Adam kernel;
the unfused chain ops.rasterization -> ops.exposure_fwd -> ops.loss_l1_ssim -> ops.exposure_bwd -> ops.blend_bwd ->
ops.project_sh_bwd for the fused step; st3r_gs_train_step for everything that must not move.  Run on the MI355X box:
    python -m pytest tests/test_gpu_exposure.py -m gpu -q -s
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from st3r_synth import synth
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _same_bits, _setup, _small_scene, _ulp_bound, dev,
                            make)

U24, U52 = 2.0 ** -24, 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def _exposures(C, seed):
    """near the identity with cross terms: gains in [0.8, 1.2], cross terms of a few percent, offsets within 0.05"""
    gen = torch.Generator().manual_seed(seed)
    E = torch.zeros(C, 3, 4)
    E[:, :, :3] = 0.03 * torch.randn((C, 3, 3), generator=gen)
    for j in range(3):
        E[:, j, j] = 0.8 + 0.4 * torch.rand(C, generator=gen)
    E[:, :, 3] = 0.1 * torch.rand((C, 3), generator=gen) - 0.05
    return E


# ---------------------------------------------------------------------------------------------------------------------
# 1. the stage kernels against float64 torch autograd
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 7, 9), (3, 32, 32), (3, 33, 32), (8, 120, 160), (256, 4, 4), (3, 768, 1024)]


@functools.lru_cache(maxsize=None)
def _stage_case(shape):
    """inputs, the float64 autograd reference and the bounds of one shape; computed once and not modified by anyone"""
    C, H, W = shape
    gen = torch.Generator().manual_seed(7000 + 100 * C + 10 * H + W)
    x = torch.rand((C, H, W, 3), generator=gen)
    vy = torch.randn((C, H, W, 3), generator=gen)
    E = _exposures(C, 31 * C + H)
    x64 = x.double().requires_grad_(); E64 = E.double().requires_grad_()
    A, t = E64[:, :, :3], E64[:, :, 3]
    y = torch.einsum("cji,chwi->chwj", A, x64) + t[:, None, None, :]
    (y * vy.double()).sum().backward()
    Aa, ta = E.double()[:, :, :3].abs(), E.double()[:, :, 3].abs()
    y_bound = 4 * U24 * (torch.einsum("cji,chwi->chwj", Aa, x.double().abs()) + ta[:, None, None, :])
    vx_bound = 4 * U24 * torch.einsum("cji,chwj->chwi", Aa, vy.double().abs())
    terms = torch.zeros((C, 3, 4), dtype=torch.float64)   # sum_p |term| of every entry of v_E
    terms[:, :, :3] = torch.einsum("chwj,chwi->cji", vy.double().abs(), x.double().abs())
    terms[:, :, 3] = vy.double().abs().sum((1, 2))
    vE_bound = U24 * E64.grad.abs() + H * W * U52 * terms
    return dict(x=x, vy=vy, E=E, y=y.detach(), vx=x64.grad, vE=E64.grad, y_bound=y_bound, vx_bound=vx_bound,
                vE_bound=vE_bound)


def _within(got, ref, bound):
    return bool(((got.double().cpu() - ref).abs() <= bound).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_stage_kernels_vs_fp64_autograd(ctx, shape):
    from starst3r_amd import ops
    R = _stage_case(shape)
    x, vy, E = R["x"].cuda(), R["vy"].cuda(), R["E"].cuda()
    y = ops.exposure_fwd(ctx, x, E)
    vx, vE = ops.exposure_bwd(ctx, x, E, vy)
    y2 = ops.exposure_fwd(ctx, x, E)
    vx2, vE2 = ops.exposure_bwd(ctx, x, E, vy)
    alias = vy.clone()
    vx3, vE3 = ops.exposure_bwd(ctx, x, E, alias, v_rgb=alias)
    torch.cuda.synchronize()
    worst = lambda got, ref, bound: float(((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(shape, "error / bound: y %.3f, v_x %.3f, v_E %.3f" % (worst(y, R["y"], R["y_bound"]), worst(vx, R["vx"], R["vx_bound"]),
                                                              worst(vE, R["vE"], R["vE_bound"])))
    assert _within(y, R["y"], R["y_bound"])
    assert _within(vx, R["vx"], R["vx_bound"])
    assert _within(vE, R["vE"], R["vE_bound"])
    assert float(vE.abs().min()) > 0
    # the same inputs give the same bits; v_rgb written over v_out gives the bits of the separate buffers
    assert _same_bits(y, y2) and _same_bits(vx, vx2) and _same_bits(vE, vE2)
    assert vx3.data_ptr() == alias.data_ptr() and _same_bits(vx3, vx) and _same_bits(vE3, vE)


def test_stage_kernels_on_unaligned_buffers(ctx):
    """(3,32,32) has H * W a multiple of 4, but buffers that start 4 bytes past a 16-byte boundary take the 4-byte path: the
    per-pixel results have the bits of the aligned call (the same float32 operations), the sums stay within their bound"""
    from starst3r_amd import ops
    R = _stage_case((3, 32, 32))
    E = R["E"].cuda()

    def off(t):
        big = torch.zeros(t.numel() + 4, device="cuda:0")
        out = big[1:1 + t.numel()].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4
        return out
    x, vy = R["x"].cuda(), R["vy"].cuda()
    y = ops.exposure_fwd(ctx, x, E)
    vx, vE = ops.exposure_bwd(ctx, x, E, vy)
    xo, vyo = off(R["x"]), off(R["vy"])
    yo = ops.exposure_fwd(ctx, xo, E, out=off(torch.zeros_like(R["x"])))
    vxo, vEo = ops.exposure_bwd(ctx, xo, E, vyo, v_rgb=vyo)
    torch.cuda.synchronize()
    assert _same_bits(yo.clone(), y) and _same_bits(vxo.clone(), vx)
    assert _within(vEo, R["vE"], R["vE_bound"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the exposure Adam kernel against float64 torch
# ---------------------------------------------------------------------------------------------------------------------
def _ref_adam(E, G, m, v, lr, step):
    E, G, m, v = E.double(), G.double(), m.double(), v.double()
    m = B1 * m + (1 - B1) * G
    v = B2 * v + (1 - B2) * G * G
    E = E - lr * (m / (1 - B1 ** step)) / ((v / (1 - B2 ** step)).sqrt() + EPS)
    return E, m, v


def _run_adam(ctx, C, steps, lr, use_mask, check):
    from starst3r_amd import ops
    gen = torch.Generator().manual_seed(200 + C)
    E = _exposures(C, 5 + C).cuda()
    m = (0.01 * torch.randn((C, 3, 4), generator=gen)).cuda()
    v = (1e-4 * torch.rand((C, 3, 4), generator=gen)).cuda()
    mask = None
    if use_mask:
        mask = torch.ones(C); mask[::3] = 0.0
        mask = mask.cuda()
    start = [t.clone() for t in (E, m, v)]
    worst = dict(E=0.0, m=0.0, v=0.0)
    for it in range(1, steps + 1):
        G = torch.randn((C, 3, 4), generator=gen).cuda()
        if check:   # the reference starts from the kernel's own float32 state: one step's rounding separates them
            rE, rm, rv = _ref_adam(E.cpu(), G.cpu(), m.cpu(), v.cpu(), lr, it)
        ops.exposure_adam_step(ctx, E, G, m.view(-1), v.view(-1), lr, B1, B2, EPS, it, mask)
        if not check:
            continue
        live = (torch.ones(C, dtype=torch.bool) if mask is None else mask.cpu() > 0)
        lv = live.numpy()
        dE = (E.cpu().double() - rE).reshape(C, -1).abs().max(dim=1).values.numpy()
        assert np.all(dE[lv] <= _ulp_bound(rE)[lv]), (C, it, dE[lv].max())
        worst["E"] = max(worst["E"], float((dE[lv] / _ulp_bound(rE, 1)[lv]).max()))
        for name, got, ref in (("m", m, rm), ("v", v, rv)):
            rel = ((got.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300))[live]
            assert float(rel.max()) <= 1e-6, (C, it, name, float(rel.max()))
            worst[name] = max(worst[name], float(rel.max()))
    torch.cuda.synchronize()
    return (E, m, v), start, mask, worst


@pytest.mark.parametrize("C", [1, 8, 256])
def test_exposure_adam_kernel_vs_fp64(ctx, C):
    end, start, mask, worst = _run_adam(ctx, C, 50, 1e-2, use_mask=C > 1, check=True)
    print(f"exposure Adam C={C}: worst E {worst['E']:.2f} ulp, m {worst['m']:.1e} rel, v {worst['v']:.1e} rel")
    if mask is not None:
        frozen = (mask == 0).cpu()
        assert int(frozen.sum()) > 0
        for a, b in zip(end, start):   # E, m, v of a masked view keep their bits
            assert _same_bits(a.cpu()[frozen], b.cpu()[frozen])
        assert not _same_bits(end[0].cpu()[~frozen], start[0].cpu()[~frozen])
    else:
        assert not _same_bits(end[0], start[0])
    again, _, _, _ = _run_adam(ctx, C, 50, 1e-2, use_mask=C > 1, check=False)
    for a, b in zip(end, again):
        assert _same_bits(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the fused-step tests
# ---------------------------------------------------------------------------------------------------------------------
class _ERun(_Run):
    """_Run plus the exposures, their gradient buffer and their moments"""

    def __init__(self, P0, vm, campos, steps, E0):
        super().__init__(P0, vm, campos, steps)
        self.E = E0.clone().contiguous()
        self.vE = torch.zeros_like(self.E)
        self.em = torch.zeros(self.E.numel(), device="cuda:0"); self.ev = torch.zeros_like(self.em)

    def state(self):
        return [self.P[k] for k in sorted(self.P)] + [self.m, self.v, self.E, self.em, self.ev, self.losses]


def _step(ctx, r, K, gt, W, H, it, lr=1e-3, exp_lr=1e-3, mask=None, want_stats=True, ssim_fac=0.2, reg=0.01):
    """train_step on whatever is registered, then the exposure update behind it"""
    from starst3r_amd import ops
    out = ops.train_step(ctx, r.P, r.vm, K, r.campos, gt, W, H, ssim_fac, reg, reg, r.grads, r.m, r.v, lr, B1, B2, EPS, it + 1,
                         r.losses[it:it + 1], want_stats=want_stats)
    ops.exposure_adam_step(ctx, r.E, r.vE, r.em, r.ev, exp_lr, B1, B2, EPS, it + 1, mask)
    return out


def _unfused(ctx, P, vm, K, gt, E, W, H, ssim_fac):
    """the unfused chain -> grads [23N], v_exposure, the loss as float32, and (rgb, v_y) for the bound of the sums"""
    from starst3r_amd import ops
    Cn = vm.shape[0]
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    y = ops.exposure_fwd(ctx, rgb, E)
    sums, v_y = ops.loss_l1_ssim(ctx, y, gt, 1.0 - ssim_fac, ssim_fac, want_grad=True)
    v_x, v_E = ops.exposure_bwd(ctx, rgb, E, v_y)
    v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                             info["_last_ids"], v_x, None, info["_cum_tiles"], Cn, W, H)
    grads = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, info["_campos"], W,
                               H, info["_splats"], v_splats)
    torch.cuda.synchronize()
    # k_finalize_loss's formula on the per-view sums, in double, stored as float32
    w_ssim = float(np.float32(ssim_fac)); w_l1 = float(np.float32(1.0) - np.float32(ssim_fac))
    inv_px = 1.0 / (float(H) * W * 3); inv_cnt = 1.0 / (float(H - 10) * (W - 10) * 3)
    s = sums.cpu().numpy()
    loss = 0.0
    for c in range(Cn):
        loss += w_l1 * s[c, 0] * inv_px + w_ssim * (1.0 - s[c, 1] * inv_cnt)
    return grads, v_E, np.float32(loss), rgb, v_y


def _fused(ctx, P, vm, K, campos, gt, E, W, H, ssim_fac, debug=0):
    from starst3r_amd import ops
    N = P["means"].shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    vE = torch.full_like(E, 7.0)
    ops.set_exposure(ctx, gt, E, vE)
    ops.set_debug(ctx, debug)
    try:
        ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, ssim_fac, 0.0, 0.0, grads, loss)
    finally:
        ops.set_debug(ctx, 0)
        ops.set_exposure(ctx, None, None, None)
    torch.cuda.synchronize()
    return grads, vE, loss


# ---------------------------------------------------------------------------------------------------------------------
# 3. fused equals unfused
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_step_equals_unfused_chain(name):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    E = _exposures(Cn, 77).cuda()
    grads_u, vE_u, loss_u, rgb, v_y = _unfused(ctx, P, vm, K, gt, E, W, H, 0.2)
    assert float(vE_u.abs().min()) > 0 and float(grads_u.abs().max()) > 0
    grads_f, vE_f, loss_f = _fused(ctx, P, vm, K, campos, gt, E, W, H, 0.2)
    print(name, "fused vs unfused: grads max |d| %.1e, v_exposure max |d| %.1e, loss %.9g vs %.9g"
          % (float((grads_f - grads_u).abs().max()), float((vE_f - vE_u).abs().max()), float(loss_f), float(loss_u)))
    assert _same_bits(grads_f, grads_u), name
    assert _same_bits(vE_f, vE_u), name
    assert np.float32(float(loss_f)).tobytes() == loss_u.tobytes(), (name, float(loss_f), float(loss_u))
    # the raw render stays where st3r_ctx_peek(8) finds it
    assert _same_bits(ops.peek(ctx, 8, rgb.numel(), torch.float32), rgb.reshape(-1))
    # the exposures do something: without a registration the gradient is another one
    grads_p = torch.empty_like(grads_u); loss_p = torch.zeros(1, device="cuda:0")
    ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads_p, loss_p)
    torch.cuda.synchronize()
    assert not _same_bits(grads_p, grads_f)
    if name == "many":   # 9 views in chunks of 4 and 5 (debug flag 32): a view belongs to one chunk, which writes its row
        grads_c, vE_c, loss_c = _fused(ctx, P, vm, K, campos, gt, E, W, H, 0.2, debug=32)
        terms = torch.zeros((Cn, 3, 4), dtype=torch.float64)
        terms[:, :, :3] = torch.einsum("chwj,chwi->cji", v_y.double().abs(), rgb.double().abs()).cpu()
        terms[:, :, 3] = v_y.double().abs().sum((1, 2)).cpu()
        bound = U24 * vE_f.double().cpu().abs() + H * W * U52 * terms   # test 1's bound (a view's chunking may differ with C)
        d = (vE_c.double().cpu() - vE_f.double().cpu()).abs()
        print("many, two view chunks: v_exposure error / bound %.3f, grads max rel %.1e"
              % (float((d / bound).max()), float((grads_c - grads_f).abs().max() / grads_f.abs().max())))
        assert bool((d <= bound).all())
        # the Gaussian gradients: the agreement of test_view_chunks_give_the_gradients_of_the_whole_call
        assert float((grads_c - grads_f).abs().max() / grads_f.abs().max()) < 1e-6
        assert float(loss_c) == pytest.approx(float(loss_f), rel=1e-6)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
def _identity(C):
    return torch.eye(3, 4, device="cuda:0").repeat(C, 1, 1).contiguous()


def test_identity_exposures_change_nothing():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P0, vm, K, campos, gt, W, H = _medium(ctx)
    Cn, steps = vm.shape[0], 5
    a = _Run(P0, vm, campos, steps)
    for it in range(steps):
        ops.train_step(ctx, a.P, a.vm, K, a.campos, gt, W, H, 0.2, 0.01, 0.01, a.grads, a.m, a.v, 1e-3, B1, B2, EPS, it + 1,
                       a.losses[it:it + 1])
        a.snaps.append(a.grads.clone())
    # identity exposures at rate 0: value equality (the identity transform may turn a -0.0 cotangent into +0.0)
    b = _ERun(P0, vm, campos, steps, _identity(Cn))
    ops.set_exposure(ctx, gt, b.E, b.vE)
    for it in range(steps):
        _step(ctx, b, K, gt, W, H, it, exp_lr=0.0)
        b.snaps.append(b.grads.clone())
    ops.set_exposure(ctx, None, None, None)
    torch.cuda.synchronize()
    for k in a.P:
        assert torch.equal(a.P[k], b.P[k]), k
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.losses, b.losses)
    for x, y in zip(a.snaps, b.snaps):
        assert torch.equal(x, y)
    assert _same_bits(b.E, _identity(Cn)) and float(b.vE.abs().max()) > 0
    # a cleared registration: the bits of plain train_step
    c = _ERun(P0, vm, campos, steps, _identity(Cn))
    ops.set_exposure(ctx, gt, c.E, c.vE)
    ops.set_exposure(ctx, None, None, None)
    for it in range(steps):
        ops.train_step(ctx, c.P, c.vm, K, c.campos, gt, W, H, 0.2, 0.01, 0.01, c.grads, c.m, c.v, 1e-3, B1, B2, EPS, it + 1,
                       c.losses[it:it + 1])
        c.snaps.append(c.grads.clone())
    torch.cuda.synchronize()
    for k in a.P:
        assert _same_bits(a.P[k], c.P[k]), k
    assert _same_bits(a.m, c.m) and _same_bits(a.v, c.v) and _same_bits(a.losses, c.losses)
    for x, y in zip(a.snaps, c.snaps):
        assert _same_bits(x, y)
    assert float(c.vE.abs().max()) == 0.0   # nobody wrote it
    # all views masked: E, m and v keep their bits while the gradient is computed and handed out
    E0 = _exposures(Cn, 3).cuda()
    d = _ERun(P0, vm, campos, steps, E0)
    d.em.copy_(0.01 * torch.randn(d.em.shape, device="cuda:0")); d.ev.copy_(1e-4 * torch.rand(d.ev.shape, device="cuda:0"))
    em0, ev0 = d.em.clone(), d.ev.clone()
    ops.set_exposure(ctx, gt, d.E, d.vE)
    for it in range(2):
        _step(ctx, d, K, gt, W, H, it, exp_lr=1e-2, mask=torch.zeros(Cn, device="cuda:0"))
    ops.set_exposure(ctx, None, None, None)
    torch.cuda.synchronize()
    assert _same_bits(d.E, E0) and _same_bits(d.em, em0) and _same_bits(d.ev, ev0)
    assert float(d.vE.abs().min()) > 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. asynchronous equals synchronous; 6. the capacity / repeat protocol
# ---------------------------------------------------------------------------------------------------------------------
def test_async_exposure_steps_equal_synchronous_steps():
    from starst3r_amd import ops
    steps = 10
    runs = []
    for want_stats in (True, False):
        ctx = ops.Context("cuda:0")   # a private context: the record-count hint is per context
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        E0 = _exposures(vm.shape[0], 9).cuda()
        r = _ERun(P0, vm, campos, steps, E0)
        ops.set_exposure(ctx, gt, r.E, r.vE)
        for it in range(steps):
            _step(ctx, r, K, gt, W, H, it, want_stats=want_stats)
        ops.settle(ctx)   # (no asynchronous step outgrew its buffers)
        torch.cuda.synchronize()
        runs.append(r)
        ctx.close()
    assert not _same_bits(runs[0].E, E0) and float(runs[0].em.abs().min()) > 0
    for x, y in zip(runs[0].state(), runs[1].state()):
        assert _same_bits(x, y)


def test_overflowing_async_exposure_step_moves_nothing_and_is_repeated():
    """debug flag 8 halves the capacity of an asynchronous step: its records past the capacity are dropped, so neither the
    Gaussians nor the exposures may move; st3r_ctx_settle reports it and the repeated step gives the undisturbed run, bit
    for bit."""
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        ctx = ops.Context("cuda:0")
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        r = _ERun(P0, vm, campos, 3, _exposures(vm.shape[0], 9).cuda())
        ops.set_exposure(ctx, gt, r.E, r.vE)
        it = 0
        while it < 3:
            before = [x.clone() for x in r.state()[:-1]] if it == overflow_at else None
            if it == overflow_at:
                ops.set_debug(ctx, 8)
            _step(ctx, r, K, gt, W, H, it, want_stats=False)
            ops.set_debug(ctx, 0)
            if it == overflow_at:
                overflow_at = -1
                with pytest.raises(_lib.St3rError) as e:
                    ops.settle(ctx)
                assert e.value.code == -3
                for x, y in zip(r.state()[:-1], before):   # Gaussians, moments, exposures, their moments: nothing moved
                    assert _same_bits(x, y)
                continue   # repeat the same iteration
            it += 1
        ops.settle(ctx)
        torch.cuda.synchronize()
        ctx.close()
        return r
    a, b = steps(-1), steps(1)
    assert float(a.em.abs().min()) > 0
    for x, y in zip(a.state(), b.state()):
        assert _same_bits(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a communicator with an applying registration
# ---------------------------------------------------------------------------------------------------------------------
def test_exposures_with_a_communicator_are_invalid():
    from starst3r_amd import dist as sdist, ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    r = _ERun(P0, vm, campos, 1, _exposures(vm.shape[0], 9).cuda())
    r.grads.fill_(7.0); r.vE.fill_(7.0)
    before = [x.clone() for x in r.state() + [r.grads, r.vE]]
    sdist.attach_native_comm(ctx)
    ops.set_exposure(ctx, gt, r.E, r.vE)
    try:
        with pytest.raises(ValueError, match="communicator"):   # ST3R_ERR_INVALID (_lib.check)
            ops.train_fwd_bwd(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.losses[0:1])
        with pytest.raises(ValueError, match="communicator"):
            ops.train_step(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, 1,
                           r.losses[0:1])
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(r.state() + [r.grads, r.vE], before))
    finally:
        ops.set_exposure(ctx, None, None, None)
        sdist.detach_native_comm(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. exposure recovery through the fused step, Gaussians frozen
# ---------------------------------------------------------------------------------------------------------------------
RECOVERY_ITERS = 300


def _recovery_lr(it):
    return 1e-4 + (1e-2 - 1e-4) * (1 + math.cos(math.pi * it / RECOVERY_ITERS)) / 2   # a cosine 1e-2 -> 1e-4


def _recovery_scene(ctx, V=3):
    from starst3r_amd import ops
    W, H = 160, 120
    g, w2c, Ks = synth.make_scene(20000, V, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    rgb, _, _ = ops.render(ctx, P, vm, K, ops.camera_positions(vm), W, H)
    return g, w2c, Ks, P, vm, K, rgb.contiguous(), W, H


def test_exposure_recovery_through_the_fused_step():
    """The scene of test_pose_recovery_through_the_fused_step; the ground truth is its render passed through known
    exposures (gains in [0.8, 1.2], cross terms of a few percent, offsets within 0.05).  Gaussian lr 0, no regularisers, no
    SSIM, exposures from the identity, view 0 frozen at its true value; 300 calls with a cosine exposure rate 1e-2 -> 1e-4.
    Measured reduction of max |E - E_true|: view 1 7.10e-02 -> 8.67e-05 (819x), view 2 1.78e-01 -> 3.83e-05 (4655x); the loss
    7.708e-02 -> 4.244e-05.  The bar asserted below is one decade under the smaller factor, 81.9 ("ends below its start",
    i.e. > 1, is asserted per view as well)."""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, P0, vm, K, rgb, W, H = _recovery_scene(ctx)
    Cn = vm.shape[0]
    E_true = _exposures(Cn, 123).cuda()
    gt = ops.exposure_fwd(ctx, rgb, E_true)
    E0 = _identity(Cn)
    E0[0] = E_true[0]
    mask = torch.ones(Cn, device="cuda:0"); mask[0] = 0.0
    r = _ERun(P0, vm, ops.camera_positions(vm), RECOVERY_ITERS, E0)
    ops.set_exposure(ctx, gt, r.E, r.vE)
    for it in range(RECOVERY_ITERS):
        _step(ctx, r, K, gt, W, H, it, lr=0.0, exp_lr=_recovery_lr(it), mask=mask, want_stats=False, ssim_fac=0.0, reg=0.0)
    ops.settle(ctx)
    ops.set_exposure(ctx, None, None, None)
    torch.cuda.synchronize()
    for k in P0:   # Gaussian lr = 0: the update is exactly zero
        assert _same_bits(r.P[k], P0[k]), k
    assert _same_bits(r.E[0], E_true[0])
    err0 = (E0 - E_true).abs().reshape(Cn, -1).max(dim=1).values.cpu().numpy()
    err1 = (r.E - E_true).abs().reshape(Cn, -1).max(dim=1).values.cpu().numpy()
    L = r.losses.cpu().numpy()
    print("exposure recovery, loss %.3e -> %.3e" % (L[0], L[-1]))
    factors = []
    for c in range(1, Cn):
        factors.append(err0[c] / err1[c])
        print("exposure recovery, view %d: max |E - E_true| %.2e -> %.2e (%.1fx)" % (c, err0[c], err1[c], factors[-1]))
        assert err1[c] < err0[c], (c, err0[c], err1[c])
    print("exposure recovery: smallest reduction factor %.2f" % min(factors))
    assert min(factors) > RECOVERY_BAR
    ctx.close()


RECOVERY_BAR = 81.9   # one decade under the smallest measured factor (819x)


# ---------------------------------------------------------------------------------------------------------------------
# 9. through run_3dgs_optim and render_3dgs
# ---------------------------------------------------------------------------------------------------------------------
OPTIM_ITERS = 200


def test_exposures_through_run_3dgs_optim(ctx):
    """The scene of check 8, photographs = the true Gaussians' render through known exposures (view 0: the identity, the
    frozen gauge), start = synth.perturb_for_gt; 200 iterations with exposure_lr 2e-3 against without.
    Measured: mean loss of the last 20 iterations 0.16083 (off) -> 0.06199 (on); max |E - E_true| of the trained views
    0.071 -> 0.045 and 0.178 -> 0.087 after these 200 iterations (the Gaussians' colours move at the same time)."""
    from starst3r_amd import ops
    g, w2c, Ks, P_true, vm, K, rgb, W, H = _recovery_scene(ctx)
    V = vm.shape[0]
    E_true = _exposures(V, 123).cuda()
    E_true[0] = _identity(1)[0]
    imgs = ops.exposure_fwd(ctx, rgb, E_true).cpu().numpy()
    g_start = synth.perturb_for_gt(g)
    off = _optim_scene(g_start, torch.tensor(w2c), Ks, imgs)
    on = _optim_scene(g_start, torch.tensor(w2c), Ks, imgs)
    losses_off = off.run_3dgs_optim(OPTIM_ITERS, exposure_lr=0.0, exposure_freeze=(0,))
    assert not hasattr(off, "exposures") and not hasattr(off._gs_optim, "exp_m")
    losses_on = on.run_3dgs_optim(OPTIM_ITERS, exposure_lr=2e-3, exposure_freeze=(0,))
    tail_off, tail_on = float(np.mean(losses_off[-20:])), float(np.mean(losses_on[-20:]))
    print("run_3dgs_optim: mean loss of the last 20 iterations %.5f (exposures off) -> %.5f (on)" % (tail_off, tail_on))
    assert len(losses_on) == OPTIM_ITERS and all(np.isfinite(losses_on)) and tail_on < tail_off
    st_ = on._gs_optim
    E = on.exposures
    assert tuple(E.shape) == (V, 3, 4) and E.dtype == torch.float32 and E.is_cuda
    assert _same_bits(E[0], _identity(1)[0]) and not _same_bits(E[1], _identity(1)[0])   # view 0 is frozen
    d0 = (_identity(V) - E_true).abs().reshape(V, -1).max(dim=1).values
    d1 = (E - E_true).abs().reshape(V, -1).max(dim=1).values
    print("run_3dgs_optim: max |E - E_true| per view", ["%.3f -> %.3f" % (float(a), float(b)) for a, b in zip(d0, d1)])
    assert st_.exp_step == OPTIM_ITERS and st_.step == OPTIM_ITERS
    em = st_.exp_m
    assert float(em.view(V, 12)[0].abs().max()) == 0.0 and float(em.view(V, 12)[1:].abs().min()) > 0
    # a second call continues the counters and the moments; a callable rate receives this call's iteration index
    seen = []
    on.run_3dgs_optim(5, exposure_lr=lambda step: seen.append(step) or 1e-4, exposure_freeze=(0,))
    assert st_.exp_step == OPTIM_ITERS + 5 and st_.exp_m is em and on.exposures is E and seen == [0, 1, 2, 3, 4]
    assert ops.get_context("cuda:0")._ex_keep is None   # the registration belongs to the call
    # together with the poses and the depth prior
    on.depth_maps = [torch.full((H, W), 3.0) for _ in range(V)]
    both = on.run_3dgs_optim(5, pose_lr=1e-5, pose_freeze=(0,), depth_fac=0.1, exposure_lr=1e-4, exposure_freeze=(0,))
    assert len(both) == 5 and all(np.isfinite(both)) and st_.exp_step == OPTIM_ITERS + 10 and st_.pose_step == 5
    pruned = on.run_3dgs_optim(3, enable_pruning=True, exposure_lr=1e-4, exposure_freeze=(0,))
    assert len(pruned) == 3 and all(np.isfinite(pruned))
    # render_3dgs_original(exposure=True): the plain render through scene.exposures
    with torch.no_grad():
        plain, _, _ = on.render_3dgs_original(W, H)
        exposed, _, _ = on.render_3dgs_original(W, H, exposure=True)
        assert _same_bits(exposed, ops.exposure_fwd(ctx, plain.contiguous(), on.exposures))
        rgbd, _, _ = on.render_3dgs_original(W, H, render_mode="RGB+ED", exposure=True)
        assert _same_bits(rgbd[..., :3].contiguous(), exposed)
    with pytest.raises(ValueError):
        off.render_3dgs_original(W, H, exposure=True)


def test_render_3dgs_back_propagates_through_the_exposures(ctx):
    """render_3dgs(exposure=E) into E, w2c and the Gaussians: the values of the unfused chain of stage calls"""
    import starst3r_amd as st
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("small")
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    Cn, N = vm.shape[0], P["means"].shape[0]
    E0 = _exposures(Cn, 41).cuda()
    gen = torch.Generator(device="cuda:0").manual_seed(8)
    V = torch.randn((Cn, H, W, 3), device="cuda:0", generator=gen)
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(v.clone()) for k, v in P.items()}
    w = vm.clone().requires_grad_(); E = E0.clone().requires_grad_()
    img, alpha, _ = scene.render_3dgs(w, K, W, H, exposure=E)
    (img * V).sum().backward()
    # the unfused chain
    rgb, alpha_u, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    assert _same_bits(img.detach(), ops.exposure_fwd(ctx, rgb, E0))
    v_x, v_E = ops.exposure_bwd(ctx, rgb, E0, V)
    vs = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha_u, info["_last_ids"],
                       v_x, None, info["_cum_tiles"], Cn, W, H)
    grads = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, info["_campos"], W,
                               H, info["_splats"], vs)
    v_vm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H, info["_splats"],
                           vs)
    torch.cuda.synchronize()
    assert float(v_E.abs().min()) > 0 and float(v_vm.abs().max()) > 0
    assert torch.equal(E.grad, v_E)
    assert torch.equal(w.grad, v_vm)
    assert torch.equal(scene.gaussians["means"].grad, ops.split_grads(grads, N)["means"])
    # the depth channel of "RGB+ED" is left alone
    with torch.no_grad():
        a, _, _ = scene.render_3dgs(vm, K, W, H, render_mode="RGB+ED")
        b, _, _ = scene.render_3dgs(vm, K, W, H, render_mode="RGB+ED", exposure=E0)
    assert _same_bits(a[..., 3].contiguous(), b[..., 3].contiguous()) and _same_bits(b[..., :3].contiguous(), img.detach())


# ---------------------------------------------------------------------------------------------------------------------
# 10. layouts without exposure training say so
# ---------------------------------------------------------------------------------------------------------------------
def test_exposure_lr_under_the_gaussian_sharded_setting_is_refused(monkeypatch):
    scene, _, _ = _small_scene(depth=None)
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, exposure_lr=1e-3)
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, exposure_lr=lambda step: 1e-3)
    assert not hasattr(scene, "exposures") and not hasattr(scene._gs_optim, "exp_m") and scene._gs_optim.step == 0


def test_exposure_lr_under_torch_distributed_is_refused(monkeypatch):
    from starst3r_amd import dist as sdist
    scene, _, _ = _small_scene(depth=None)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, exposure_lr=1e-3)
    assert not hasattr(scene, "exposures") and not hasattr(scene._gs_optim, "exp_m") and scene._gs_optim.step == 0
