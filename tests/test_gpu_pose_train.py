"""Camera poses inside the fused training step: st3r_pose_adam_step (gs_pose_step.hip), st3r_gs_train_step_poses and
run_3dgs_optim(pose_lr=..., pose_freeze=...).

References: the update rule restated in float64 torch for the kernel; the unfused chain ops.rasterization ->
ops.loss_l1_ssim -> ops.blend_bwd -> ops.viewmat_bwd for the fused pose gradient; st3r_gs_train_step for everything
that must not move.  Run on the MI355X box:
    python -m pytest tests/test_gpu_pose_train.py -m gpu -q -s
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from st3r_synth import synth
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _pose_errors, _same_bits, _se3_exp, _setup,
                            _ulp_bound, dev, make, rel_err_per_camera)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the pose Adam kernel against float64 torch
# ---------------------------------------------------------------------------------------------------------------------
def _hat(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def _ref_pose_step(V, G, m, v, lr, step):
    """the update rule of include/st3r.h in float64: V [C,4,4], G [C,4,4], m / v [C,6] -> V', campos', m', v'"""
    V, G, m, v = V.double(), G.double(), m.double(), v.double()
    R, t = V[:, :3, :3], V[:, :3, 3]
    GR, Gt = G[:, :3, :3], G[:, :3, 3]
    A = GR @ R.transpose(1, 2)
    g_om = torch.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], -1) + \
        torch.linalg.cross(t, Gt)
    g = torch.cat([g_om, Gt], -1)
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    delta = -lr * (m / (1 - B1 ** step)) / ((v / (1 - B2 ** step)).sqrt() + EPS)
    E = torch.linalg.matrix_exp(_hat(delta[:, :3]))   # Rodrigues
    Rn = E @ R
    tn = (E @ t[:, :, None])[:, :, 0] + delta[:, 3:]
    r0 = Rn[:, 0] / Rn[:, 0].norm(dim=-1, keepdim=True)
    r1 = Rn[:, 1] - (Rn[:, 1] * r0).sum(-1, keepdim=True) * r0
    r1 = r1 / r1.norm(dim=-1, keepdim=True)
    r2 = torch.linalg.cross(r0, r1)
    Rn = torch.stack([r0, r1, r2], 1)
    Vn = torch.zeros_like(V)
    Vn[:, :3, :3] = Rn; Vn[:, :3, 3] = tn; Vn[:, 3, 3] = 1.0
    campos = -(Rn.transpose(1, 2) @ tn[:, :, None])[:, :, 0]
    return Vn, campos, m, v


def _random_rigid(C, gen):
    w = torch.randn((C, 3), dtype=torch.float64, generator=gen)
    R = torch.linalg.matrix_exp(_hat(w))
    V = torch.zeros((C, 4, 4), dtype=torch.float64)
    V[:, :3, :3] = R; V[:, :3, 3] = 3.0 * torch.randn((C, 3), dtype=torch.float64, generator=gen); V[:, 3, 3] = 1.0
    return V


def _run_kernel_steps(ctx, C, steps, lr, use_mask, check):
    from starst3r_amd import ops
    gen = torch.Generator().manual_seed(100 + C)
    V0 = _random_rigid(C, gen)
    V = V0.float().cuda()
    campos = (-(V0[:, :3, :3].transpose(1, 2) @ V0[:, :3, 3:4])[:, :, 0]).float().cuda()
    m = (0.01 * torch.randn((C, 6), generator=gen)).cuda()
    v = (1e-4 * torch.rand((C, 6), generator=gen)).cuda()
    mask = None
    if use_mask:
        mask = torch.ones(C); mask[::3] = 0.0
        mask = mask.cuda()
    start = [x.clone() for x in (V, campos, m, v)]
    worst = dict(V=0.0, campos=0.0, m=0.0, v=0.0)
    for it in range(1, steps + 1):
        G = torch.randn((C, 4, 4), generator=gen).cuda()   # row 3 is random too: the kernel must ignore it
        if check:   # the reference starts from the kernel's own float32 state: one step's rounding separates them
            rV, rc, rm, rv = _ref_pose_step(V.cpu(), G.cpu(), m.cpu(), v.cpu(), lr, it)
        ops.pose_adam_step(ctx, V, campos, G, m.view(-1), v.view(-1), lr, B1, B2, EPS, it, mask)
        if not check:
            continue
        live = torch.ones(C, dtype=torch.bool) if mask is None else mask.cpu() > 0
        dV = (V.cpu().double() - rV).reshape(C, -1).abs().max(dim=1).values.numpy()
        dc = (campos.cpu().double() - rc).abs().max(dim=1).values.numpy()
        lv = live.numpy()
        assert np.all(dV[lv] <= _ulp_bound(rV)[lv]), (C, it, dV[lv].max())
        assert np.all(dc[lv] <= _ulp_bound(rc)[lv]), (C, it, dc[lv].max())
        for name, got, ref in (("m", m, rm), ("v", v, rv)):
            rel = ((got.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300))[live]
            assert float(rel.max()) <= 1e-6, (C, it, name, float(rel.max()))
            worst[name] = max(worst[name], float(rel.max()))
        worst["V"] = max(worst["V"], float((dV[lv] / (_ulp_bound(rV, 1)[lv])).max()))
        worst["campos"] = max(worst["campos"], float((dc[lv] / (_ulp_bound(rc, 1)[lv])).max()))
    torch.cuda.synchronize()
    return (V, campos, m, v), start, mask, worst


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


@pytest.mark.parametrize("C", [1, 8, 256])
def test_pose_adam_kernel_vs_fp64(ctx, C):
    end, start, mask, worst = _run_kernel_steps(ctx, C, 50, 1e-2, use_mask=C > 1, check=True)
    print(f"pose Adam C={C}: worst V {worst['V']:.2f} ulp, campos {worst['campos']:.2f} ulp, "
          f"m {worst['m']:.1e} rel, v {worst['v']:.1e} rel")
    V = end[0].cpu().double()
    R = V[:, :3, :3]
    orth = float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max())
    print(f"pose Adam C={C}: |R R^T - I|_max after 50 steps = {orth:.1e}")
    assert orth <= 1e-6
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0])
    assert torch.equal(end[0][:, 3].cpu(), bottom.expand(C, 4))
    if mask is not None:
        frozen = (mask == 0).cpu()
        assert int(frozen.sum()) > 0
        for a, b in zip(end, start):   # V, campos, m, v of a masked camera keep their bits
            assert _same_bits(a.cpu()[frozen], b.cpu()[frozen])
        assert not _same_bits(end[0].cpu()[~frozen], start[0].cpu()[~frozen])
    # the same inputs give the same bits
    again, _, _, _ = _run_kernel_steps(ctx, C, 50, 1e-2, use_mask=C > 1, check=False)
    for a, b in zip(end, again):
        assert _same_bits(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the fused-step tests
# ---------------------------------------------------------------------------------------------------------------------
def _unfused_pose_grad(ctx, P, vm, K, gt, W, H, ssim_fac):
    from starst3r_amd import ops
    Cn = vm.shape[0]
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    _, v_rgb = ops.loss_l1_ssim(ctx, rgb, gt, 1.0 - ssim_fac, ssim_fac, want_grad=True)
    v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                             info["_last_ids"], v_rgb, None, info["_cum_tiles"], Cn, W, H)
    out = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H,
                          info["_splats"], v_splats)
    torch.cuda.synchronize()
    return out


def _step_poses(ctx, r, K, gt, W, H, it, lr=1e-3, pose_lr=1e-3, mask=None, want_stats=True, ssim_fac=0.2, reg=0.01):
    from starst3r_amd import ops
    return ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, ssim_fac, reg, reg, r.grads, r.m, r.v, lr, B1, B2,
                                EPS, it + 1, r.losses[it:it + 1], r.pm, r.pv, pose_lr, it + 1, mask, r.vvm,
                                want_stats=want_stats)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused pose gradient equals the unfused composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_pose_gradient_equals_unfused_chain(name):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    ref = _unfused_pose_grad(ctx, P0, vm, K, gt, W, H, 0.2)
    assert float(ref.abs().max()) > 0
    r = _Run(P0, vm, campos, 1)
    _step_poses(ctx, r, K, gt, W, H, 0)
    torch.cuda.synchronize()
    err = rel_err_per_camera(r.vvm, ref)
    print(name, "fused vs unfused pose gradient, max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    # bar: the one test_render_w2c_grad_vs_dense_fp64 gives the unfused path against float64.
    # measured: 0.0 on all four scenes -- the fused route runs the stand-alone kernels on the same slots: the same bits
    assert max(err) <= 5e-5, (name, err)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_poses_change_nothing():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P0, vm, K, campos, gt, W, H = _medium(ctx)
    steps = 5
    a = _Run(P0, vm, campos, steps)
    for it in range(steps):
        ops.train_step(ctx, a.P, a.vm, K, a.campos, gt, W, H, 0.2, 0.01, 0.01, a.grads, a.m, a.v, 1e-3, B1, B2, EPS, it + 1,
                       a.losses[it:it + 1])
        a.snaps.append(a.grads.clone())
    b = _Run(P0, vm, campos, steps)
    mask = torch.zeros(vm.shape[0], device="cuda:0")
    for it in range(steps):
        _step_poses(ctx, b, K, gt, W, H, it, mask=mask)
        b.snaps.append(b.grads.clone())
    torch.cuda.synchronize()
    for k in a.P:
        assert _same_bits(a.P[k], b.P[k]), k
    assert _same_bits(a.m, b.m) and _same_bits(a.v, b.v) and _same_bits(a.losses, b.losses)
    for x, y in zip(a.snaps, b.snaps):
        assert _same_bits(x, y)
    assert _same_bits(b.vm, vm) and _same_bits(b.campos, campos)
    assert float(b.pm.abs().max()) == 0.0 and float(b.pv.abs().max()) == 0.0
    assert float(b.vvm.abs().max()) > 0   # the gradient is still computed and handed out
    # poses on: the first step's Gaussian gradients are train_step's, and the cameras move
    c = _Run(P0, vm, campos, 1)
    _step_poses(ctx, c, K, gt, W, H, 0)
    torch.cuda.synchronize()
    assert _same_bits(c.grads, a.snaps[0])
    assert not _same_bits(c.vm, vm) and not _same_bits(c.campos, campos)
    inv = torch.inverse(c.vm.double())[:, :3, 3]
    assert float((inv - c.campos.double()).abs().max()) < 1e-5
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. asynchronous equals synchronous; chunked views; the capacity / repeat protocol
# ---------------------------------------------------------------------------------------------------------------------
def test_async_pose_steps_equal_synchronous_steps():
    from starst3r_amd import ops
    steps = 10
    runs = []
    for want_stats in (True, False):
        ctx = ops.Context("cuda:0")   # a private context: the record-count hint is per context
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        r = _Run(P0, vm, campos, steps)
        for it in range(steps):
            _step_poses(ctx, r, K, gt, W, H, it, want_stats=want_stats)
        ops.settle(ctx)   # (no asynchronous step outgrew its buffers)
        torch.cuda.synchronize()
        runs.append(r)
        ctx.close()
    assert not _same_bits(runs[0].vm, vm)
    for x, y in zip(runs[0].state(), runs[1].state()):
        assert _same_bits(x, y)


def test_chunked_views_give_the_pose_gradient_of_the_whole_call():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("many")   # 9 views: chunks of 4 and 5
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    ref = _unfused_pose_grad(ctx, P0, vm, K, gt, W, H, 0.2)
    ops.set_debug(ctx, 32)
    r = _Run(P0, vm, campos, 1)
    _step_poses(ctx, r, K, gt, W, H, 0)
    ops.set_debug(ctx, 0)
    torch.cuda.synchronize()
    err = rel_err_per_camera(r.vvm, ref)
    print("two view chunks, fused vs unfused pose gradient per camera:", ["%.1e" % e for e in err])
    assert max(err) <= 5e-5, err   # measured 0.0: a camera's gradient is computed inside its own chunk
    # every camera moved once
    one = _Run(P0, vm, campos, 1)
    ctx1 = ops.Context("cuda:0")
    _step_poses(ctx1, one, K, gt, W, H, 0)
    torch.cuda.synchronize()
    assert float((one.vm - r.vm).abs().max()) < 1e-6 and not _same_bits(r.vm, vm)
    ctx.close(); ctx1.close()


def test_overflowing_async_pose_step_moves_nothing_and_is_repeated():
    """debug flag 8 halves the capacity of an asynchronous step: its records past the capacity are dropped, so neither
    update may happen; st3r_ctx_settle reports it and the repeated step gives the undisturbed run, bit for bit."""
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        ctx = ops.Context("cuda:0")
        P0, vm, K, campos, gt, W, H = _medium(ctx)
        r = _Run(P0, vm, campos, 3)
        it = 0
        while it < 3:
            before = [x.clone() for x in r.state()[:-1]] if it == overflow_at else None
            if it == overflow_at:
                ops.set_debug(ctx, 8)
            _step_poses(ctx, r, K, gt, W, H, it, want_stats=False)
            ops.set_debug(ctx, 0)
            if it == overflow_at:
                overflow_at = -1
                with pytest.raises(_lib.St3rError) as e:
                    ops.settle(ctx)
                assert e.value.code == -3
                for x, y in zip(r.state()[:-1], before):   # Gaussians, moments, cameras, pose moments: nothing moved
                    assert _same_bits(x, y)
                continue   # repeat the same iteration
            it += 1
        ops.settle(ctx)
        torch.cuda.synchronize()
        ctx.close()
        return r
    a, b = steps(-1), steps(1)
    for x, y in zip(a.state(), b.state()):
        assert _same_bits(x, y)


def test_bad_pose_step_is_refused_before_anything_runs(ctx):
    """argument checks: a pose step counter below 1 is refused before anything runs"""
    g, w2c, Ks, W, H = make("small")
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    r = _Run(P0, vm, campos, 1)
    from starst3r_amd import ops
    with pytest.raises(ValueError):
        ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, 1,
                             r.losses[0:1], r.pm, r.pv, 1e-3, 0)
    torch.cuda.synchronize()
    assert _same_bits(r.vm, vm) and _same_bits(r.P["means"], P0["means"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. pose recovery through the fused step, Gaussians frozen
# ---------------------------------------------------------------------------------------------------------------------
def _perturb(w_true, seed, degrees, frac, baseline):
    """as test_pose_recovery perturbs its camera: a rotation about a random axis, the centre moved along a random direction"""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
    dirn = rng.standard_normal(3); dirn /= np.linalg.norm(dirn)
    rot = _se3_exp(torch.tensor(np.r_[axis * math.radians(degrees), 0, 0, 0]))
    w = rot @ w_true
    R = w[:3, :3]
    w[:3, 3] = -R @ (-R.T @ w[:3, 3] + torch.tensor(dirn * frac * baseline))
    return w


def _baseline(w2c):
    c0 = -w2c[0, :3, :3].T.astype(np.float64) @ w2c[0, :3, 3]; c1 = -w2c[1, :3, :3].T.astype(np.float64) @ w2c[1, :3, 3]
    return float(np.linalg.norm(c1 - c0))


def test_pose_recovery_through_the_fused_step():
    """The scene of test_pose_recovery, all three cameras perturbed (2 degrees, 2 % of the baseline), Gaussian lr = 0:
    200 calls of train_step_poses with that test's cosine schedule bring every camera back by more than 100x.
    Seeds: camera 1 keeps that test's perturbation (seed 5); cameras 2 and 0 take the next two seeds (6, 7).
    Measured (rotation / centre reduction): camera 0 1448x / 568x, camera 1 1940x / 1460x, camera 2 671x / 962x.
    Recorded as well: with the seeds 5, 6, 7 on cameras 0, 1, 2 the third camera reaches 5.0x / 2.7x only -- and so does
    the route of test_pose_recovery itself (torch Adam on an se(3) twist through render_3dgs autograd) on that camera and
    perturbation: 5.1x / 2.8x, the same trajectory within 1 % at every 25th step.  That case is slow for the schedule,
    not for the fused step."""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    W, H = 160, 120
    g, w2c, Ks = synth.make_scene(20000, 3, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    P0 = {k: dev(v) for k, v in g.items()}
    vm_true, K = dev(w2c), dev(Ks)
    gt, _, _ = ops.render(ctx, P0, vm_true, K, ops.camera_positions(vm_true), W, H)
    gt = gt.contiguous()
    base = _baseline(w2c)
    w_true = [torch.tensor(w2c[c], dtype=torch.float64) for c in range(3)]
    w_pert = torch.stack([_perturb(w_true[c], 5 + (c - 1) % 3, 2.0, 0.02, base) for c in range(3)])
    err0 = [_pose_errors(w_pert[c], w_true[c]) for c in range(3)]
    vm = w_pert.float().cuda().contiguous()
    campos = ops.camera_positions(vm)
    iters = 200
    r = _Run(P0, vm, campos, iters)
    for it in range(iters):
        pose_lr = 2e-4 + (2e-3 - 2e-4) * (1 + math.cos(math.pi * it / iters)) / 2   # CosineAnnealingLR(T_max=200, eta_min=2e-4)
        _step_poses(ctx, r, K, gt, W, H, it, lr=0.0, pose_lr=pose_lr, want_stats=False, ssim_fac=0.0, reg=0.0)
    ops.settle(ctx)
    torch.cuda.synchronize()
    for k in P0:   # Gaussian lr = 0: the update is exactly zero
        assert _same_bits(r.P[k], P0[k]), k
    err1 = [_pose_errors(r.vm[c].cpu().double(), w_true[c]) for c in range(3)]
    for c in range(3):
        print("fused pose recovery, camera %d: rotation %.2e -> %.2e rad (%.0fx), centre %.2e -> %.2e (%.0fx)"
              % (c, err0[c][0], err1[c][0], err0[c][0] / err1[c][0], err0[c][1], err1[c][1], err0[c][1] / err1[c][1]))
    L = r.losses.cpu().numpy()
    print("fused pose recovery, loss %.3e -> %.3e" % (L[0], L[-1]))
    for c in range(3):
        assert err1[c][0] < err0[c][0] / 100 and err1[c][1] < err0[c][1] / 100, (c, err0[c], err1[c])
    # the hard assignment of the docstring (seeds 5, 6, 7 on cameras 0, 1, 2), printed and not asserted: a change there
    # stays visible in the output
    w_hard = torch.stack([_perturb(w_true[c], 5 + c, 2.0, 0.02, base) for c in range(3)])
    e0 = [_pose_errors(w_hard[c], w_true[c]) for c in range(3)]
    vm_h = w_hard.float().cuda().contiguous()
    rh = _Run(P0, vm_h, ops.camera_positions(vm_h), iters)
    for it in range(iters):
        pose_lr = 2e-4 + (2e-3 - 2e-4) * (1 + math.cos(math.pi * it / iters)) / 2
        _step_poses(ctx, rh, K, gt, W, H, it, lr=0.0, pose_lr=pose_lr, want_stats=False, ssim_fac=0.0, reg=0.0)
    ops.settle(ctx)
    torch.cuda.synchronize()
    e1 = [_pose_errors(rh.vm[c].cpu().double(), w_true[c]) for c in range(3)]
    for c in range(3):
        print("fused pose recovery, seeds 5 6 7 (not asserted), camera %d: rotation %.1fx, centre %.1fx"
              % (c, e0[c][0] / e1[c][0], e0[c][1] / e1[c][1]))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. joint refinement through run_3dgs_optim
# ---------------------------------------------------------------------------------------------------------------------
JOINT_ITERS = 5000
JOINT_LR = 2e-3   # a cosine from JOINT_LR to JOINT_LR / 10: the rates of test_pose_recovery's schedule (2e-3 -> 2e-4)


def _joint_pose_lr(step):
    return 0.1 * JOINT_LR + 0.9 * JOINT_LR * (1 + math.cos(math.pi * step / JOINT_ITERS)) / 2


def test_joint_refinement_through_run_3dgs_optim(ctx):
    """Four views, the true Gaussians through synth.perturb_for_gt, cameras 1-3 off by 1 degree and 1 % of the baseline,
    camera 0 frozen; 5000 iterations, pose_lr a cosine 2e-3 -> 2e-4 over them (Gaussian lr 1e-3, the default).
    Measured with these settings, in a run made as ten run_3dgs_optim calls of 500 iterations each so that the errors could
    be read on the way (scene.c2w passes through float32 between the calls; the single call below was not measured
    separately): mean loss of the last 20 iterations 0.04571 (poses off) -> 0.04469 (poses on); reduction factors
    rotation / centre: camera 1 3.56x / 1.44x, camera 2 3.69x / 2.71x, camera 3 3.33x / 1.36x.  Smallest factor 1.36; the
    bar asserted below is one decade under it, 0.136 (the issue's "ends below its start", i.e. > 1, is asserted per camera
    and is the sharper of the two).
    Why these settings: the Gaussians start with re-drawn colours and move at 1e-3 per step themselves, so whatever pose
    error the cameras have not removed early the Gaussians fit around (they absorb it), and it comes back out slowly.  The
    cameras therefore start at once and at the rate that recovers them against frozen Gaussians (2e-3, check 5), and the
    run is long enough for the centres to follow the rotations.  Measured on the way (iterations / iterations held at zero
    rate / peak rate -> smallest factor): 1500/0/5e-4 0.98, 1500/0/2e-3 1.08, 1500/0/5e-3 0.97, 5000/0/5e-4 1.05,
    5000/0/1e-4 constant 0.66, 10000/0/2e-3 1.56, 10000/2000/2e-3 0.64, 20000/0/1e-3 1.75, 3000/1000/5e-4 0.7: a slow or
    late start is what loses the centres; a longer run keeps gaining.  The result IS sensitive to the settings: most of the
    neighbours above end within 10 % of 1.0 or under it, and the margin here (1.36 against the 1.0 the issue asks for) is
    not wide; it grew monotonically over the run (0.97 at 500 iterations, 1.13 at 1500, 1.26 at 3000, 1.36 at 5000)."""
    from starst3r_amd import ops
    W, H, V = 160, 120, 4
    g, w2c, Ks = synth.make_scene(20000, V, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    P_true = {k: dev(v) for k, v in g.items()}
    vm_true = dev(w2c)
    imgs, _, _ = ops.render(ctx, P_true, vm_true, dev(Ks), ops.camera_positions(vm_true), W, H)
    imgs = imgs.cpu().numpy()
    g_start = synth.perturb_for_gt(g)
    base = _baseline(w2c)
    w_true = [torch.tensor(w2c[c], dtype=torch.float64) for c in range(V)]
    w_start = torch.stack([w_true[0]] + [_perturb(w_true[c], 40 + c, 1.0, 0.01, base) for c in range(1, V)])
    err0 = [_pose_errors(w_start[c], w_true[c]) for c in range(V)]
    off = _optim_scene(g_start, w_start, Ks, imgs)
    on = _optim_scene(g_start, w_start, Ks, imgs)
    c2w_before = on.c2w
    w2c_before = on.w2c.clone()
    losses_off = off.run_3dgs_optim(JOINT_ITERS)
    losses_on = on.run_3dgs_optim(JOINT_ITERS, pose_lr=_joint_pose_lr, pose_freeze=(0,))
    assert off.c2w is not on.c2w and torch.equal(off.c2w, c2w_before)   # poses off: c2w is left alone
    tail_off, tail_on = float(np.mean(losses_off[-20:])), float(np.mean(losses_on[-20:]))
    print("joint refinement: mean loss of the last 20 iterations %.5f (poses off) -> %.5f (poses on)" % (tail_off, tail_on))
    assert tail_on < tail_off
    st_ = on._gs_optim
    refined = st_.pose_w2c.detach().cpu().double()
    err1 = [_pose_errors(refined[c], w_true[c]) for c in range(V)]
    factors = []
    for c in range(1, V):
        fr, fc = err0[c][0] / err1[c][0], err0[c][1] / err1[c][1]
        factors += [fr, fc]
        print("joint refinement, camera %d: rotation %.2e -> %.2e rad (%.1fx), centre %.2e -> %.2e (%.1fx)"
              % (c, err0[c][0], err1[c][0], fr, err0[c][1], err1[c][1], fc))
        assert err1[c][0] < err0[c][0] and err1[c][1] < err0[c][1], (c, err0[c], err1[c])
    print("joint refinement: smallest reduction factor %.2f" % min(factors))
    assert min(factors) > 0.136   # one decade under the measured 1.36
    # scene.c2w: a new tensor, device and dtype as before, the inverse of the refined matrices
    assert on.c2w is not c2w_before and on.c2w.dtype == c2w_before.dtype and on.c2w.device == c2w_before.device
    assert float((torch.inverse(on.c2w.double()) - refined).abs().max()) <= 1e-5
    assert float((on.w2c.double().cpu() - refined).abs().max()) <= 1e-5   # the w2c cache refreshed itself
    # camera 0 is frozen: bit-unchanged, in the trained matrices and in c2w
    assert _same_bits(st_.pose_w2c[0].cpu(), w2c_before[0].float().cpu())
    assert _same_bits(on.c2w[0], c2w_before[0])
    # the pose state persists: a second call continues from it
    assert st_.pose_step == JOINT_ITERS and st_.step == JOINT_ITERS
    pm = st_.pose_m
    assert float(pm.view(V, 6)[0].abs().max()) == 0.0 and float(pm.view(V, 6)[1:].abs().max()) > 0
    on.run_3dgs_optim(5, pose_lr=1e-5, pose_freeze=(0,))
    assert st_.pose_step == JOINT_ITERS + 5 and st_.pose_m is pm
    assert not hasattr(off._gs_optim, "pose_m")


# ---------------------------------------------------------------------------------------------------------------------
# 7. layouts without pose training say so
# ---------------------------------------------------------------------------------------------------------------------
def test_pose_lr_under_the_gaussian_sharded_setting_is_refused(monkeypatch):
    g, w2c, Ks, W, H = make("small")
    imgs = np.zeros((w2c.shape[0], H, W, 3), np.float32)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
    c2w = scene.c2w
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, pose_lr=1e-3)
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, pose_lr=lambda step: 1e-3)
    assert scene.c2w is c2w and not hasattr(scene._gs_optim, "pose_m")


def test_pose_lr_under_torch_distributed_is_refused(monkeypatch):
    """world > 1: refused before any GPU work (the process group is not needed to see it: rank_world is what the loop asks)"""
    from starst3r_amd import dist as sdist
    g, w2c, Ks, W, H = make("small")
    imgs = np.zeros((w2c.shape[0], H, W, 3), np.float32)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
    c2w = scene.c2w
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, pose_lr=1e-3)
    assert scene.c2w is c2w and not hasattr(scene._gs_optim, "pose_m") and scene._gs_optim.step == 0


def test_train_step_poses_with_a_communicator_is_invalid():
    """st3r_gs_train_step_poses on a context with a communicator attached (one rank is enough): ST3R_ERR_INVALID with a
    message, nothing written"""
    from starst3r_amd import dist as sdist, ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    r = _Run(P0, vm, campos, 1)
    before = [x.clone() for x in r.state()]
    sdist.attach_native_comm(ctx)
    try:
        with pytest.raises(ValueError, match="communicator"):   # ST3R_ERR_INVALID (_lib.check)
            _step_poses(ctx, r, K, gt, W, H, 0)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(r.state(), before))
    finally:
        sdist.detach_native_comm(ctx)
        ctx.close()
