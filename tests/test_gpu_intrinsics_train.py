"""Intrinsics inside the fused training step: st3r_intrinsics_adam_step and st3r_ctx_set_intrinsics_grad
(gs_intrinsics.hip) and run_3dgs_optim with scene.intrinsics_lr, scene.intrinsics_freeze set.

References: the update rule restated in float64 torch for the Adam kernel; the unfused chain ops.rasterization ->
ops.loss_l1_ssim -> ops.blend_bwd -> ops.intrinsics_bwd (with exposures and a depth prior: the stand-alone calls the fused
step makes) for the registered gradient; st3r_gs_train_step for everything that must not move.  Run on the MI355X box:
    python -m pytest tests/test_gpu_intrinsics_train.py -m gpu -q -s
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from st3r_synth import synth
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _same_bits, _setup, _synthetic_prior, dev, make)

DEPTH_FAC = 0.5


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the intrinsics Adam kernel against float64 torch
# ---------------------------------------------------------------------------------------------------------------------
AW, AH = 640, 480


def _ref_k_step(K, G, m, v, lr, step, mode):
    """the update rule of include/st3r.h in float64: K [C,3,3], G [C,4], m / v [C,4] -> K', m', v'"""
    K, G, m, v = K.double().clone(), G.double(), m.double().clone(), v.double().clone()
    fx, fy = K[:, 0, 0], K[:, 1, 1]
    g = torch.stack([fx * G[:, 0], fy * G[:, 1], AW * G[:, 2], AH * G[:, 3]], -1)
    if mode & 1:
        g[:, 0] = g[:, 0] + g[:, 1]
    live = [0] if mode & 1 else [0, 1]
    if mode & 2:
        live += [2, 3]
    delta = torch.zeros_like(g)
    for q in live:
        m[:, q] = B1 * m[:, q] + (1 - B1) * g[:, q]
        v[:, q] = B2 * v[:, q] + (1 - B2) * g[:, q] * g[:, q]
        delta[:, q] = -lr * (m[:, q] / (1 - B1 ** step)) / ((v[:, q] / (1 - B2 ** step)).sqrt() + EPS)
    K[:, 0, 0] = fx * torch.exp(delta[:, 0])
    K[:, 1, 1] = fy * torch.exp(delta[:, 0] if mode & 1 else delta[:, 1])
    K[:, 0, 2] = K[:, 0, 2] + AW * delta[:, 2]
    K[:, 1, 2] = K[:, 1, 2] + AH * delta[:, 3]
    return K, m, v


def _random_K(C, gen):
    K = torch.randn((C, 3, 3), generator=gen)   # skew and row 2 hold noise: the kernel must not touch them
    fx = 50.0 + 1950.0 * torch.rand(C, generator=gen)
    K[:, 0, 0] = fx; K[:, 1, 1] = fx * (0.9 + 0.2 * torch.rand(C, generator=gen))
    K[:, 0, 2] = AW * (0.4 + 0.2 * torch.rand(C, generator=gen)); K[:, 1, 2] = AH * (0.4 + 0.2 * torch.rand(C, generator=gen))
    return K


def _run_adam(ctx, C, steps, lr, mode, use_mask, check):
    from starst3r_amd import ops
    gen = torch.Generator().manual_seed(100 + C)
    K = _random_K(C, gen).cuda()
    m = (0.01 * torch.randn((C, 4), generator=gen)).cuda()
    v = (1e-4 * torch.rand((C, 4), generator=gen)).cuda()
    mask = None
    if use_mask:
        mask = torch.ones(C); mask[::3] = 0.0
        mask = mask.cuda()
    start = [x.clone() for x in (K, m, v)]
    worst = dict(K=0.0, m=0.0, v=0.0)
    scale = torch.tensor([1.0, 1.0, 1.0 / AW, 1.0 / AH])
    for it in range(1, steps + 1):
        G = (torch.randn((C, 4), generator=gen) * scale / 100.0).cuda()   # g = O(1) for the focals, O(0.01) for pp
        if check:   # the reference starts from the kernel's own float32 state: one step's rounding separates them
            rK, rm, rv = _ref_k_step(K.cpu(), G.cpu(), m.cpu(), v.cpu(), lr, it, mode)
        ops.intrinsics_adam_step(ctx, K, G, m.view(-1), v.view(-1), lr, B1, B2, EPS, it, mask, AW, AH, bool(mode & 1),
                                 bool(mode & 2))
        if not check:
            continue
        live = torch.ones(C, dtype=torch.bool) if mask is None else mask.cpu() > 0
        # K: the float32 store of a double result -- half an ulp; one more for exp() of the device against torch's
        d = (K.cpu().double() - rK).abs()[live]
        ulp = torch.tensor(np.spacing(rK.abs().float().numpy()).astype(np.float64))[live]
        assert bool((d <= 1.5 * ulp).all()), (C, mode, it, float((d / ulp).max()))
        worst["K"] = max(worst["K"], float((d / ulp).max()))
        for name, got, ref in (("m", m, rm), ("v", v, rv)):
            rel = ((got.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300))[live]
            assert float(rel.max()) <= 1e-6, (C, mode, it, name, float(rel.max()))
            worst[name] = max(worst[name], float(rel.max()))
    torch.cuda.synchronize()
    return (K, m, v), start, mask, worst


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [1, 5, 64, 65])   # the edges of ceil_div(C, 64) workgroups of 64 threads
def test_intrinsics_adam_kernel_vs_fp64(ctx, C, mode):
    steps = 20
    end, start, mask, worst = _run_adam(ctx, C, steps, 1e-2, mode, use_mask=C > 1, check=True)
    print(f"intrinsics Adam C={C} mode={mode}: worst K {worst['K']:.2f} ulp, m {worst['m']:.1e} rel, v {worst['v']:.1e} rel")
    K1, m1, v1 = (x.cpu() for x in end)
    K0, m0, v0 = (x.cpu() for x in start)
    live = torch.ones(C, dtype=torch.bool) if mask is None else mask.cpu() > 0
    if mask is not None:
        assert int((~live).sum()) > 0
        for a, b in zip((K1, m1, v1), (K0, m0, v0)):   # K, m, v of a masked view keep their bits
            assert _same_bits(a[~live], b[~live])
    # the live views moved
    assert not _same_bits(K1[live][:, 0, 0], K0[live][:, 0, 0]) and not _same_bits(K1[live][:, 1, 1], K0[live][:, 1, 1])
    # skew and row 2 are never written
    for i, j in ((0, 1), (1, 0), (2, 0), (2, 1), (2, 2)):
        assert _same_bits(K1[:, i, j], K0[:, i, j]), (i, j)
    if mode & 2:
        assert not _same_bits(K1[live][:, 0, 2], K0[live][:, 0, 2]) and not _same_bits(K1[live][:, 1, 2], K0[live][:, 1, 2])
    else:   # without bit 1 the principal point and its moments keep every bit
        assert _same_bits(K1[:, 0, 2], K0[:, 0, 2]) and _same_bits(K1[:, 1, 2], K0[:, 1, 2])
        assert _same_bits(m1[:, 2:], m0[:, 2:]) and _same_bits(v1[:, 2:], v0[:, 2:])
    if mode & 1:
        # tied: moment slot 1 is not touched, and fx / fy is kept -- each step rounds fx and fy to float32 once, half an
        # ulp (2^-24 relative) each, so the ratio moves by at most 2^-23 per step
        assert _same_bits(m1[:, 1], m0[:, 1]) and _same_bits(v1[:, 1], v0[:, 1])
        r0 = K0[:, 0, 0].double() / K0[:, 1, 1].double(); r1 = K1[:, 0, 0].double() / K1[:, 1, 1].double()
        drift = float((r1 / r0 - 1.0).abs().max())
        print(f"intrinsics Adam C={C} mode={mode}: fx / fy moved by {drift:.1e} relative over {steps} steps")
        assert drift <= steps * 2.0 ** -23
    # the same inputs give the same bits
    again, _, _, _ = _run_adam(ctx, C, steps, 1e-2, mode, use_mask=C > 1, check=False)
    for a, b in zip(end, again):
        assert _same_bits(a, b)


@pytest.mark.parametrize("mode", [0, 2])
def test_untied_focal_without_a_gradient_keeps_its_bits(ctx, mode):
    from starst3r_amd import ops
    C = 5
    gen = torch.Generator().manual_seed(7)
    K = _random_K(C, gen).cuda()
    K0 = K.clone()
    m = torch.zeros(4 * C, device="cuda:0"); v = torch.zeros_like(m)
    for it in range(1, 6):
        G = (torch.randn((C, 4), generator=gen) / 100.0).cuda()
        G[:, 1] = 0.0   # no gradient reaches fy
        ops.intrinsics_adam_step(ctx, K, G, m, v, 1e-2, B1, B2, EPS, it, None, AW, AH, False, bool(mode & 2))
    torch.cuda.synchronize()
    assert _same_bits(K[:, 1, 1], K0[:, 1, 1]) and not _same_bits(K[:, 0, 0], K0[:, 0, 0])
    assert float(m.view(C, 4)[:, 1].abs().max()) == 0.0 and float(v.view(C, 4)[:, 1].abs().max()) == 0.0


def test_bad_intrinsics_step_is_refused(ctx):
    from starst3r_amd import ops
    K = _random_K(2, torch.Generator().manual_seed(1)).cuda()
    K0 = K.clone()
    z = torch.zeros(8, device="cuda:0")
    with pytest.raises(ValueError):
        ops.intrinsics_adam_step(ctx, K, z.view(2, 4), z.clone(), z.clone(), 1e-3, B1, B2, EPS, 0, None, AW, AH)
    with pytest.raises(ValueError):
        ops.intrinsics_adam_step(ctx, K, z.view(2, 4), z.clone(), z.clone(), 1e-3, 1.0, B2, EPS, 1, None, AW, AH)
    torch.cuda.synchronize()
    assert _same_bits(K, K0)


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the fused-step tests
# ---------------------------------------------------------------------------------------------------------------------
def _exposures(C, seed):
    gen = torch.Generator().manual_seed(seed)
    E = torch.eye(3, 4).repeat(C, 1, 1) + 0.1 * torch.randn((C, 3, 4), generator=gen)
    return E.contiguous()


def _unfused(ctx, P, vm, K, gt, W, H, ssim_fac=0.2, E=None, prior=None):
    """the stand-alone calls the fused step makes, in its order -> (v_Ks [C,4], v_viewmats [C,4,4]) of the per-pair
    gradients (with a depth prior: the summed ones; row 2 of v_viewmats without the depth column)"""
    from starst3r_amd import ops
    Cn = vm.shape[0]
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    y = rgb if E is None else ops.exposure_fwd(ctx, rgb, E)
    _, v_x = ops.loss_l1_ssim(ctx, y, gt, 1.0 - ssim_fac, ssim_fac, want_grad=True)
    if E is not None:
        v_x, _ = ops.exposure_bwd(ctx, rgb, E, v_x)
    v_a = v_d = None
    if prior is not None:
        d = ops.blend_depth_fwd(ctx, *lists, alpha, info["_last_ids"], Cn, W, H)
        _, v_d, v_a = ops.loss_depth_prior(ctx, d, alpha, prior[0], prior[1], DEPTH_FAC)
    ops.blend_fwd(ctx, *lists, Cn, W, H)
    vs = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_x, v_a, info["_cum_tiles"], Cn, W, H)
    if prior is not None:
        vs.add_(ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], v_d, info["_cum_tiles"], Cn, W, H))
    vK = ops.intrinsics_bwd(ctx, P["means"], P["quats"], P["scales"], vm, K, W, H, info["_splats"], vs)
    vvm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H, info["_splats"], vs)
    torch.cuda.synchronize()
    return vK, vvm


def _step(ctx, r, gt, W, H, it, poses=False, k_lr=1e-3, mask=None, want_stats=True, adam=True):
    """train_step (or train_step_poses) on whatever is registered, then the intrinsics update behind it"""
    from starst3r_amd import ops
    if poses:
        out = ops.train_step_poses(ctx, r.P, r.vm, r.K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2,
                                   EPS, it + 1, r.losses[it:it + 1], r.pm, r.pv, 1e-3, it + 1, None, r.vvm,
                                   want_stats=want_stats)
    else:
        out = ops.train_step(ctx, r.P, r.vm, r.K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS,
                             it + 1, r.losses[it:it + 1], want_stats=want_stats)
    if adam:   # untied focals and the principal point: all four moment slots are in use
        ops.intrinsics_adam_step(ctx, r.K, r.vK, r.km, r.kv, k_lr, B1, B2, EPS, it + 1, mask, W, H, False, True)
    return out


def _fused_vK(ctx, P, vm, K, campos, gt, W, H, debug=0, want_stats=True):
    """st3r_gs_train_fwd_bwd with the registration -> (v_Ks, grads, loss)"""
    from starst3r_amd import ops
    N, Cn = P["means"].shape[0], vm.shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    vK = torch.full((Cn, 4), 7.0, device="cuda:0")
    ops.set_intrinsics_grad(ctx, gt, vK)
    ops.set_debug(ctx, debug)
    try:
        ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads, loss, want_stats=want_stats)
    finally:
        ops.set_debug(ctx, 0)
        ops.set_intrinsics_grad(ctx, None, None)
    torch.cuda.synchronize()
    return vK, grads, loss


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the registered gradient is the unfused chain's; nothing else changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_intrinsics_gradient_equals_unfused_chain(name):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    ref, _ = _unfused(ctx, P, vm, K, gt, W, H)
    assert float(ref.abs().min()) > 0
    vK, grads, loss = _fused_vK(ctx, P, vm, K, campos, gt, W, H)
    print(name, "fused vs unfused intrinsics gradient, max |d| / max |ref|: %.1e" % _rel(vK, ref))
    # measured: 0.0 on all four scenes -- the fused route runs the stand-alone kernels on the same slots: the same bits
    assert _same_bits(vK, ref), name
    # the Gaussians' gradients and the loss are those of a call without the registration
    grads_p = torch.empty_like(grads); loss_p = torch.zeros(1, device="cuda:0")
    ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads_p, loss_p)
    torch.cuda.synchronize()
    assert _same_bits(grads, grads_p) and _same_bits(loss, loss_p)
    # asynchronous (the second call without statistics leaves the record count on the device): the same gradient
    _fused_vK(ctx, P, vm, K, campos, gt, W, H, want_stats=False)
    vK_a, grads_a, _ = _fused_vK(ctx, P, vm, K, campos, gt, W, H, want_stats=False)
    ops.settle(ctx)
    assert _same_bits(vK_a, ref) and _same_bits(grads_a, grads_p)
    if name == "many":   # 9 views in chunks of 4 and 5 (debug flag 32): a view belongs to one chunk, which writes its row
        vK_c, grads_c, loss_c = _fused_vK(ctx, P, vm, K, campos, gt, W, H, debug=32)
        print("many, two view chunks: intrinsics gradient max |d| / max |ref| %.1e" % _rel(vK_c, ref))
        assert _same_bits(vK_c, ref)   # measured 0.0: a camera's gradient is computed inside its own chunk
        assert float((grads_c - grads_p).abs().max() / grads_p.abs().max()) < 1e-6
    ctx.close()


def test_registration_combines_with_poses_depth_prior_and_exposures():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    E = _exposures(Cn, 77).cuda()
    prior = _synthetic_prior(ctx, P, vm, K, W, H)[:2]
    plain, plain_vm = _unfused(ctx, P, vm, K, gt, W, H)

    def fused(poses, with_E, with_prior, register=True):
        r = _Run(P, vm, campos, 1, K)
        vE = torch.zeros_like(E)
        if with_E:
            ops.set_exposure(ctx, gt, E, vE)
        if with_prior:
            ops.set_depth_prior(ctx, gt, prior[0], prior[1], DEPTH_FAC)
        if register:
            ops.set_intrinsics_grad(ctx, gt, r.vK)
        try:
            _step(ctx, r, gt, W, H, 0, poses=poses, adam=False)
        finally:
            ops.set_exposure(ctx, None, None, None); ops.set_depth_prior(ctx, None, None, None)
            ops.set_intrinsics_grad(ctx, None, None)
        torch.cuda.synchronize()
        return r

    # poses on: the intrinsics gradient of the unfused chain, and the pose gradient keeps its bits
    r = fused(True, False, False)
    assert _same_bits(r.vK, plain) and _same_bits(r.vvm, plain_vm)
    r0 = fused(True, False, False, register=False)
    for x, y in zip(r.state(), r0.state()):
        assert _same_bits(x, y)
    assert float((r0.vK - 7.0).abs().max()) == 0.0   # without the registration nothing is written
    # exposures; a depth prior (the summed per-pair gradients); all of it together
    for poses, with_E, with_prior in ((False, True, False), (False, False, True), (True, True, True)):
        ref, _ = _unfused(ctx, P, vm, K, gt, W, H, E=E if with_E else None, prior=prior if with_prior else None)
        r = fused(poses, with_E, with_prior)
        print("poses %d exposures %d depth prior %d: max |d| / max |ref| %.1e" % (poses, with_E, with_prior, _rel(r.vK, ref)))
        assert _same_bits(r.vK, ref), (poses, with_E, with_prior)   # measured 0.0
        assert not _same_bits(ref, plain)
        r0 = fused(poses, with_E, with_prior, register=False)
        for x, y in zip(r.state(), r0.state()):
            assert _same_bits(x, y)
    ctx.close()


def test_cleared_registration_changes_nothing():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P0, vm, K, campos, gt, W, H = _medium(ctx)
    steps = 3
    a = _Run(P0, vm, campos, steps, K)
    for it in range(steps):
        _step(ctx, a, gt, W, H, it, adam=False)
    b = _Run(P0, vm, campos, steps, K)
    ops.set_intrinsics_grad(ctx, gt, b.vK)
    ops.set_intrinsics_grad(ctx, None, None)
    for it in range(steps):
        _step(ctx, b, gt, W, H, it, adam=False)
    # registered, with every view masked: the gradient is written, nothing moves
    c = _Run(P0, vm, campos, steps, K)
    ops.set_intrinsics_grad(ctx, gt, c.vK)
    mask = torch.zeros(vm.shape[0], device="cuda:0")
    for it in range(steps):
        _step(ctx, c, gt, W, H, it, mask=mask)
    ops.set_intrinsics_grad(ctx, None, None)
    torch.cuda.synchronize()
    for x, y, z in zip(a.state(), b.state(), c.state()):
        assert _same_bits(x, y) and _same_bits(x, z)
    assert float((b.vK - 7.0).abs().max()) == 0.0 and float(c.vK.abs().min()) > 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. asynchronous equals synchronous; the capacity / repeat protocol; a communicator
# ---------------------------------------------------------------------------------------------------------------------
def test_async_intrinsics_steps_equal_synchronous_steps():
    from starst3r_amd import ops
    steps = 10
    runs = []
    for want_stats in (True, False):
        ctx = ops.Context("cuda:0")   # a private context: the record-count hint is per context
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        r = _Run(P0, vm, campos, steps, K)
        ops.set_intrinsics_grad(ctx, gt, r.vK)
        for it in range(steps):
            _step(ctx, r, gt, W, H, it, poses=True, want_stats=want_stats)
        ops.settle(ctx)   # (no asynchronous step outgrew its buffers)
        torch.cuda.synchronize()
        runs.append(r)
        ctx.close()
    assert not _same_bits(runs[0].K, K) and float(runs[0].km.abs().min()) > 0
    for x, y in zip(runs[0].state(), runs[1].state()):
        assert _same_bits(x, y)


def test_overflowing_async_intrinsics_step_moves_nothing_and_is_repeated():
    """debug flag 8 halves the capacity of an asynchronous step: its records past the capacity are dropped, so neither the
    Gaussians nor the intrinsics may move; st3r_ctx_settle reports it and the repeated step gives the undisturbed run, bit
    for bit."""
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        ctx = ops.Context("cuda:0")
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        r = _Run(P0, vm, campos, 3, K)
        ops.set_intrinsics_grad(ctx, gt, r.vK)
        it = 0
        while it < 3:
            before = [x.clone() for x in r.state()[:-1]] if it == overflow_at else None
            if it == overflow_at:
                ops.set_debug(ctx, 8)
            _step(ctx, r, gt, W, H, it, want_stats=False)
            ops.set_debug(ctx, 0)
            if it == overflow_at:
                overflow_at = -1
                with pytest.raises(_lib.St3rError) as e:
                    ops.settle(ctx)
                assert e.value.code == -3
                for x, y in zip(r.state()[:-1], before):   # Gaussians, moments, intrinsics, their moments: nothing moved
                    assert _same_bits(x, y)
                continue   # repeat the same iteration
            it += 1
        ops.settle(ctx)
        torch.cuda.synchronize()
        ctx.close()
        return r
    a, b = steps(-1), steps(1)
    assert float(a.km.abs().min()) > 0
    for x, y in zip(a.state(), b.state()):
        assert _same_bits(x, y)


def test_intrinsics_gradient_with_a_communicator_is_invalid():
    from starst3r_amd import dist as sdist, ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    r = _Run(P0, vm, campos, 1, K)
    r.grads.fill_(7.0)
    before = [x.clone() for x in r.state() + [r.grads, r.vK]]
    sdist.attach_native_comm(ctx)
    ops.set_intrinsics_grad(ctx, gt, r.vK)
    try:
        with pytest.raises(ValueError, match="communicator"):   # ST3R_ERR_INVALID (_lib.check)
            ops.train_fwd_bwd(ctx, r.P, r.vm, r.K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.losses[0:1])
        with pytest.raises(ValueError, match="communicator"):
            ops.train_step(ctx, r.P, r.vm, r.K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, 1,
                           r.losses[0:1])
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(r.state() + [r.grads, r.vK], before))
    finally:
        ops.set_intrinsics_grad(ctx, None, None)
        sdist.detach_native_comm(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. run_3dgs_optim with scene.intrinsics_lr
# ---------------------------------------------------------------------------------------------------------------------
OPTIM_ITERS = 300
OPTIM_LR = 2e-3


def _optim_lr(step):
    return 0.1 * OPTIM_LR + 0.9 * OPTIM_LR * (1 + math.cos(math.pi * step / OPTIM_ITERS)) / 2   # a cosine 2e-3 -> 2e-4


def test_focal_refinement_through_run_3dgs_optim(ctx):
    """Three views of the true Gaussians rendered at the true intrinsics; the run starts from synth.perturb_for_gt with the
    focals of views 1 and 2 off by +3 % and -3 % (fx and fy alike), view 0 frozen at the truth; 300 iterations,
    intrinsics_lr a cosine 2e-3 -> 2e-4 (Gaussian lr 1e-3, the default).
    Measured: mean loss of the last 20 iterations 0.05615 (intrinsics off) -> 0.05491 (on); relative focal error of view 1
    3.00e-2 -> 5.71e-3 (5.3x), of view 2 3.00e-2 -> 3.37e-3 (8.9x) -- the Gaussians, which move at the same time, absorb
    part of the error.  Smallest factor 5.25; the bar asserted below is one decade under it."""
    from starst3r_amd import ops
    W, H, V = 160, 120, 3
    g, w2c, Ks = synth.make_scene(20000, V, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    P_true = {k: dev(v) for k, v in g.items()}
    vm = dev(w2c)
    imgs, _, _ = ops.render(ctx, P_true, vm, dev(Ks), ops.camera_positions(vm), W, H)
    imgs = imgs.cpu().numpy()
    g_start = synth.perturb_for_gt(g)
    Ks_start = Ks.copy()
    for c, f in ((1, 1.03), (2, 0.97)):
        Ks_start[c, 0, 0] *= f; Ks_start[c, 1, 1] *= f
    off = _optim_scene(g_start, w2c, Ks_start, imgs)
    on = _optim_scene(g_start, w2c, Ks_start, imgs)
    K_off, K_before = off.intrinsics, on.intrinsics
    off.intrinsics_freeze = (0,)   # (the rate stays at its default, 0.0: off)
    losses_off = off.run_3dgs_optim(OPTIM_ITERS)
    assert off.intrinsics is K_off and not hasattr(off._gs_optim, "k_m")   # off: scene.intrinsics is left alone
    on.intrinsics_lr, on.intrinsics_freeze = _optim_lr, (0,)
    losses_on = on.run_3dgs_optim(OPTIM_ITERS)
    tail_off, tail_on = float(np.mean(losses_off[-20:])), float(np.mean(losses_on[-20:]))
    print("focal refinement: mean loss of the last 20 iterations %.5f (off) -> %.5f (on)" % (tail_off, tail_on))
    assert len(losses_on) == OPTIM_ITERS and all(np.isfinite(losses_on)) and tail_on < tail_off
    # scene.intrinsics: a new tensor, device and dtype as before; view 0 is frozen: its row keeps every bit
    K_new = on.intrinsics
    assert K_new is not K_before and K_new.dtype == K_before.dtype and K_new.device == K_before.device
    assert tuple(K_new.shape) == (V, 3, 3) and _same_bits(K_new[0], K_before[0])
    assert torch.equal(K_before, torch.tensor(Ks_start))   # the old tensor was not trained in place
    factors = []
    for c in range(1, V):
        e0 = abs(float(Ks_start[c, 0, 0]) / float(Ks[c, 0, 0]) - 1.0)
        e1 = max(abs(float(K_new[c, 0, 0]) / float(Ks[c, 0, 0]) - 1.0), abs(float(K_new[c, 1, 1]) / float(Ks[c, 1, 1]) - 1.0))
        factors.append(e0 / max(e1, 1e-30))
        print("focal refinement, view %d: relative focal error %.2e -> %.2e (%.1fx)" % (c, e0, e1, factors[-1]))
        assert e1 < e0, (c, e0, e1)
        # tied focals: fx / fy as it was; the principal point is not trained
        assert abs(float(K_new[c, 0, 0] / K_new[c, 1, 1]) / float(Ks_start[c, 0, 0] / Ks_start[c, 1, 1]) - 1.0) <= OPTIM_ITERS * 2.0 ** -23
        assert _same_bits(K_new[c, :, 2], K_before[c, :, 2]) and _same_bits(K_new[c, 2], K_before[c, 2])
    print("focal refinement: smallest reduction factor %.2f" % min(factors))
    assert min(factors) > 0.525   # one decade under the measured 5.25
    # the state persists: a second call continues the moments and the step counter
    st_ = on._gs_optim
    assert st_.k_step == OPTIM_ITERS and st_.step == OPTIM_ITERS
    km = st_.k_m
    assert float(km.view(V, 4)[0].abs().max()) == 0.0 and float(km.view(V, 4)[1:, 0].abs().min()) > 0
    assert float(km.view(V, 4)[:, 1:].abs().max()) == 0.0   # tied, no principal point: slot 0 only
    seen = []
    on.intrinsics_lr = lambda step: seen.append(step) or 1e-5
    on.run_3dgs_optim(5)
    assert st_.k_step == OPTIM_ITERS + 5 and st_.k_m is km and seen == [0, 1, 2, 3, 4]
    assert _same_bits(on.intrinsics[0], K_before[0])
    assert ops.get_context("cuda:0")._kg_keep is None   # the registration belongs to the call
    # together with the poses, the depth prior, the exposures and pruning; untied focals and the principal point
    on.depth_maps = [torch.full((H, W), 3.0) for _ in range(V)]
    on.intrinsics_lr, on.intrinsics_tie_focal, on.intrinsics_opt_pp = 1e-5, False, True
    both = on.run_3dgs_optim(5, pose_lr=1e-5, pose_freeze=(0,), depth_fac=0.1, exposure_lr=1e-4, exposure_freeze=(0,))
    assert len(both) == 5 and all(np.isfinite(both)) and st_.k_step == OPTIM_ITERS + 10 and st_.pose_step == 5
    assert float(st_.k_m.view(V, 4)[1:].abs().min()) > 0 and float(st_.k_m.view(V, 4)[0].abs().max()) == 0.0
    assert not _same_bits(on.intrinsics[1, :, 2], K_before[1, :, 2])
    pruned = on.run_3dgs_optim(3, enable_pruning=True)
    assert len(pruned) == 3 and all(np.isfinite(pruned))
