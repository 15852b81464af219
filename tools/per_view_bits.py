"""One hash per output array of everything the per-view options of the fused 3DGS step compute, on seeded inputs: the gate
"same bits" of a refactor of that layer.  Run it on a build of the parent commit and on the tree under review (it uses the
package of the tree it lies in) and compare the two listings; run it twice on one tree to see which arrays that tree itself
does not reproduce (the colour loss adds its sums with atomics).

    python tools/per_view_bits.py > bits.txt

Covers the stage calls (loss_depth_prior, exposure_fwd / _bwd, pose_adam_step, exposure_adam_step), the fused calls
(train_fwd_bwd, train_step, train_step_poses; with a depth prior, with exposures, with both, with neither; whole and in two
view chunks) on the scenes of tests/test_gpu_pose_grad.py and tests/test_gpu_pose_train.py, run_3dgs_optim with all three
options and render_3dgs with a backward."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import starst3r_amd as st   # noqa: E402
from starst3r_amd import ops   # noqa: E402
from st3r_synth import synth   # noqa: E402
from test_gpu_pose_grad import make   # noqa: E402
from test_gpu_pose_train import _optim_scene, _setup   # noqa: E402

B1, B2, EPS = 0.9, 0.999, 1e-8


def show(tag, *tensors):
    for i, t in enumerate(tensors):
        t = torch.as_tensor(t)
        h = hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
        print(f"{tag}[{i}] {tuple(t.shape)} {h}", flush=True)


def off(t):
    """a copy of t that starts 4 bytes past a 16-byte boundary"""
    big = torch.zeros(t.numel() + 4, device="cuda:0", dtype=t.dtype)
    out = big[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def rand(gen, *shape):
    return torch.rand(shape, generator=gen).cuda()


def exposures(C, gen):
    return (torch.eye(3, 4) + 0.1 * torch.randn((C, 3, 4), generator=gen)).cuda().contiguous()


def stage_calls(ctx):
    for shape in [(1, 1, 1), (1, 17, 33), (3, 16, 64), (2, 37, 130)]:
        gen = torch.Generator().manual_seed(sum(shape))
        D, a = rand(gen, *shape, 1), 0.25 + 0.75 * rand(gen, *shape, 1)
        Z, w = 0.5 + rand(gen, *shape), rand(gen, *shape)
        w[rand(gen, *shape) < 0.3] = 0.0
        a.view(-1)[::7] = 0.0
        show(f"loss_depth_prior {shape}", *ops.loss_depth_prior(ctx, D, a, Z, w, 0.5))
        if shape == (3, 16, 64):
            show(f"loss_depth_prior {shape} unaligned", *ops.loss_depth_prior(ctx, off(D), off(a), off(Z), off(w), 0.5))
    for shape in [(1, 1, 1), (1, 3, 5), (2, 7, 9), (3, 32, 32), (3, 33, 32), (8, 120, 160), (256, 4, 4), (3, 768, 1024)]:
        gen = torch.Generator().manual_seed(sum(shape))
        x, vy, E = rand(gen, *shape, 3), torch.randn((*shape, 3), generator=gen).cuda(), exposures(shape[0], gen)
        show(f"exposure_fwd {shape}", ops.exposure_fwd(ctx, x, E))
        show(f"exposure_bwd {shape}", *ops.exposure_bwd(ctx, x, E, vy))
        if shape == (3, 32, 32):
            show(f"exposure_fwd {shape} unaligned", ops.exposure_fwd(ctx, off(x), E, out=off(x)))
            show(f"exposure_bwd {shape} unaligned", *ops.exposure_bwd(ctx, off(x), E, off(vy)))
        g = vy.clone()
        show(f"exposure_bwd {shape} in place", *ops.exposure_bwd(ctx, x, E, g, v_rgb=g))
    for C in (1, 8, 256):
        for use_mask in (False, True):
            gen = torch.Generator().manual_seed(C)
            mask = (torch.rand(C, generator=gen) > 0.4).float().cuda() if use_mask else None
            # poses
            V = torch.eye(4).repeat(C, 1, 1)
            q = torch.linalg.qr(torch.randn((C, 3, 3), generator=gen)).Q
            V[:, :3, :3] = q * torch.linalg.det(q)[:, None, None]
            V[:, :3, 3] = torch.randn((C, 3), generator=gen)
            V = V.cuda().contiguous()
            campos = ops.camera_positions(V)
            pm, pv = torch.zeros(6 * C, device="cuda:0"), torch.zeros(6 * C, device="cuda:0")
            E = exposures(C, gen)
            em, ev = torch.zeros(12 * C, device="cuda:0"), torch.zeros(12 * C, device="cuda:0")
            for step in (1, 2, 3):
                G = (0.1 * torch.randn((C, 4, 4), generator=gen)).cuda()
                ops.pose_adam_step(ctx, V, campos, G, pm, pv, 1e-2, B1, B2, EPS, step, mask)
                show(f"pose_adam C={C} mask={use_mask} step {step}", V, campos, pm, pv)
                GE = (0.1 * torch.randn((C, 3, 4), generator=gen)).cuda()
                ops.exposure_adam_step(ctx, E, GE, em, ev, 1e-2, B1, B2, EPS, step, mask)
                show(f"exposure_adam C={C} mask={use_mask} step {step}", E, em, ev)


def prior_of(ctx, P, vm, K, W, H):
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    d = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                            info["_last_ids"], vm.shape[0], W, H)
    ed = (d / alpha.clamp(min=1e-10))[..., 0]
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    Z = ed * (1 + 0.05 * torch.randn(ed.shape, device="cuda:0", generator=gen))
    w = ((alpha[..., 0] > 0.05) & (torch.rand(ed.shape, device="cuda:0", generator=gen) > 0.33)).float()
    return Z.contiguous(), w.contiguous()


def fused_calls(name):
    ctx = ops.Context("cuda:0")
    if name == "medium":
        W, H = 320, 240
        g, w2c, Ks = synth.make_scene(20000, 3, W, H, seed=5, scale_lo=0.004, scale_hi=0.03)
    else:
        g, w2c, Ks, W, H = make(name)
    P0, vm0, K, campos0, gt = _setup(ctx, g, w2c, Ks, W, H)
    Z, w = prior_of(ctx, P0, vm0, K, W, H)
    N, C = P0["means"].shape[0], vm0.shape[0]
    E = exposures(C, torch.Generator().manual_seed(3))
    for option in ("neither", "prior", "exposure", "both"):
        for debug in (0, 32):
            tag = f"{name} {option} chunks={1 + debug // 32}"
            vE = torch.zeros_like(E)
            if option in ("prior", "both"):
                ops.set_depth_prior(ctx, gt, Z, w, 0.5)
            if option in ("exposure", "both"):
                ops.set_exposure(ctx, gt, E, vE)
            ops.set_debug(ctx, debug)
            grads, loss = torch.empty(23 * N, device="cuda:0"), torch.zeros(5, device="cuda:0")
            ops.train_fwd_bwd(ctx, P0, vm0, K, campos0, gt, W, H, 0.2, 0.01, 0.01, grads, loss[0:1])
            show(tag + " train_fwd_bwd", grads, vE)
            P = {k: v.clone() for k, v in P0.items()}
            m, v = torch.zeros_like(grads), torch.zeros_like(grads)
            for it in range(2):
                ops.train_step(ctx, P, vm0, K, campos0, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, it + 1,
                               loss[1 + it:2 + it])
            show(tag + " train_step x2", grads, m, v, vE, *[P[k] for k in sorted(P)])
            P = {k: v.clone() for k, v in P0.items()}
            vm, campos = vm0.clone(), campos0.clone()
            m, v = torch.zeros_like(grads), torch.zeros_like(grads)
            pm, pv, vvm = torch.zeros(6 * C, device="cuda:0"), torch.zeros(6 * C, device="cuda:0"), torch.zeros_like(vm)
            for it in range(2):
                ops.train_step_poses(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, it + 1,
                                     loss[3 + it:4 + it], pm, pv, 1e-3, it + 1, None, vvm)
            show(tag + " train_step_poses x2", grads, m, v, vE, vm, campos, pm, pv, vvm, *[P[k] for k in sorted(P)])
            show(tag + " losses", loss)
            ops.set_debug(ctx, 0)
            ops.set_depth_prior(ctx, None, None, None)
            ops.set_exposure(ctx, None, None, None)
    ctx.close()


def python_calls():
    g, w2c, Ks, W, H = make("small")
    ctx = ops.get_context("cuda:0")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Z, _ = prior_of(ctx, P, vm, K, W, H)
    for pruning in (False, True):
        scene = _optim_scene(g, torch.tensor(w2c), Ks, gt.cpu().numpy())
        scene.depth_maps = [Z[i].cpu() for i in range(Z.shape[0])]
        losses = scene.run_3dgs_optim(20, enable_pruning=pruning, pose_lr=1e-3, pose_freeze=(0,), depth_fac=0.5,
                                      exposure_lr=1e-3, exposure_freeze=(0,))
        s = scene._gs_optim
        show(f"run_3dgs_optim pruning={pruning}", torch.tensor(losses), *[scene.gaussians[k] for k in sorted(scene.gaussians)],
             scene.c2w, scene.exposures, s.m, s.v, s.pose_m, s.pose_v, s.exp_m, s.exp_v)
    for mode in ("RGB", "RGB+ED"):
        for with_exposure in (False, True):
            scene = _optim_scene(g, torch.tensor(w2c), Ks, gt.cpu().numpy())
            w = vm.clone().requires_grad_()
            E = exposures(vm.shape[0], torch.Generator().manual_seed(5)).requires_grad_() if with_exposure else None
            img, alpha, _ = scene.render_3dgs(w, K, W, H, render_mode=mode, exposure=E)
            gen = torch.Generator(device="cuda:0").manual_seed(9)
            ((img * torch.randn(img.shape, device="cuda:0", generator=gen)).sum() + alpha.sum()).backward()
            show(f"render_3dgs {mode} exposure={with_exposure}", img, alpha, w.grad,
                 *[scene.gaussians[k].grad for k in ("means", "quats", "scales", "opacities", "shN")],
                 *([E.grad] if with_exposure else []))


if __name__ == "__main__":
    assert torch.cuda.is_available()
    stage_calls(ops.get_context("cuda:0"))
    for name in ("small", "many", "wide", "medium"):
        fused_calls(name)
    python_calls()
