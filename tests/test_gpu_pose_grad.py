"""Camera-pose gradients: st3r_gs_viewmat_bwd (gs_pose_bwd.hip) and render_3dgs back-propagating into w2c / Scene.c2w
(gsplat returns v_viewmats whenever viewmats require a gradient).

The references are float64 torch autograd: through oracle/gs_torch_ref's projection and SH colour for the kernel in
isolation, through its dense renderer end to end.  Run on the MI355X box:
    python -m pytest tests/test_gpu_pose_grad.py -m gpu -q
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gs_torch_ref as tr
from st3r_synth import synth
from per_view_cases import (_gen, _pose_errors, _se3_exp, dev, make, masked_cotangents, rel_err_per_camera,
                            run_hip)


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha):
    """HIP v_splats of the rasterization, then the kernel under test"""
    from starst3r_amd import ops
    Cn = w2c.shape[0]
    v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                             info["_last_ids"], v_rgb, v_alpha, info["_cum_tiles"], Cn, W, H)
    vm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], dev(w2c), dev(Ks), info["_campos"], W, H,
                         info["_splats"], v_splats)
    torch.cuda.synchronize()
    return v_splats, vm


def chain_ref(g, w2c, Ks, W, H, splats, v_splats):
    """float64 autograd of (means2d, conic, colour) of the visible pairs into viewmats, with
    campos = inverse(viewmats)[:3, 3] and the HIP per-pair gradients as cotangents; vectorised over each camera's pairs"""
    N, Cn = g["means"].shape[0], w2c.shape[0]
    rad = splats[:, 10].view(torch.int32).reshape(Cn, N).cpu()
    vs = v_splats.reshape(Cn, N, 12).double().cpu()
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    means, quats, scales, sh = t(g["means"]), t(g["quats"]), t(g["scales"]), t(g["shN"])
    vm = t(w2c).requires_grad_()
    K = t(Ks)
    campos = torch.inverse(vm)[:, :3, 3]
    outs, cots = [], []
    for c in range(Cn):
        idx = torch.nonzero(rad[c] > 0).reshape(-1)
        if idx.numel() == 0:
            continue
        m2, _, conic = tr.project(means[idx], quats[idx], scales[idx], vm[c], K[c], W, H)
        col = tr.sh_color(means[idx], campos[c], sh[idx])
        outs += [m2, conic, col]
        cots += [vs[c, idx, 0:2], vs[c, idx, 3:6], vs[c, idx, 6:9]]
    if not outs:
        return torch.zeros((Cn, 4, 4), dtype=torch.float64)
    (gv,) = torch.autograd.grad(outs, vm, cots)
    return gv


FUZZ3 = ["fuzz0", "fuzz1", "fuzz2"]


@pytest.mark.parametrize("name", ["small", "ragged", "medium", "one", "many", "wide"] + FUZZ3)
def test_kernel_vs_fp64_chain_rule(ctx, name):
    g, w2c, Ks, W, H = make(name)
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_splats, vm = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, dev(v_rgb), dev(v_alpha))
    ref = chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats)
    assert float(ref.abs().max()) > 0
    err = rel_err_per_camera(vm, ref)
    print(name, "max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    # measured: regular scenes <= 1.6e-7, fuzz scenes <= 2.8e-4 (fuzz0: Gaussians right in front of the camera, whose
    # 1/z^3 terms the float32 per-pair arithmetic carries)
    tol = 1e-3 if name.startswith("fuzz") else 1e-6
    assert max(err) < tol, (name, err)


@pytest.mark.parametrize("name", ["small", "ragged", "one", "many"])
def test_render_w2c_grad_vs_dense_fp64(ctx, name):
    import starst3r_amd as st
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H, seed=11)
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    w = dev(w2c).requires_grad_()
    rgb, alpha, _ = scene.render_3dgs(w, dev(Ks), W, H)
    ((rgb * dev(v_rgb)).sum() + (alpha * dev(v_alpha)).sum()).backward()
    info = ops.last_info()
    N, Cn = g["means"].shape[0], w2c.shape[0]
    rad = info["_splats"][:, 10].view(torch.int32).reshape(Cn, N).cpu().to(torch.int64)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    vm = t(w2c).requires_grad_()
    rgb_t, alpha_t = tr.render_dense(t(g["means"]), t(g["quats"]), t(g["scales"]), t(g["opacities"]), t(g["shN"]), vm,
                                     t(Ks), W, H, rad > 0, rad)
    ((rgb_t * t(v_rgb)).sum() + (alpha_t * t(v_alpha)).sum()).backward()
    err = rel_err_per_camera(w.grad, vm.grad)
    print(name, "end to end, max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    assert max(err) <= 5e-5, (name, err)   # measured <= 8.4e-6


def test_pose_gradient_changes_nothing_else(ctx):
    import starst3r_amd as st
    g, w2c, Ks, W, H = make("small")
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    v_rgb = torch.randn((w2c.shape[0], H, W, 3), device="cuda:0", generator=_gen(1))
    grads = []
    for pose_grad in (False, True):
        for p in scene.gaussians.values():
            p.grad = None
        w = dev(w2c).requires_grad_(pose_grad)
        K = dev(Ks).requires_grad_()
        rgb, alpha, _ = scene.render_3dgs(w, K, W, H)
        ((rgb * v_rgb).sum() + alpha.sum()).backward()
        assert (w.grad is not None) == pose_grad
        assert K.grad is None
        grads.append({k: p.grad.clone() for k, p in scene.gaussians.items() if p.grad is not None})
        if pose_grad:
            assert float(w.grad.abs().max()) > 0
            v_w = w.grad.clone()
    assert grads[0].keys() == grads[1].keys() and "means" in grads[0]
    for k in grads[0]:
        assert torch.equal(grads[0][k].view(torch.int32), grads[1][k].view(torch.int32)), k
    # a float64 CPU w2c gets its gradient back in its own dtype and device (autograd through render_3dgs' .to())
    for p in scene.gaussians.values():
        p.grad = None
    w64 = torch.tensor(w2c, dtype=torch.float64).requires_grad_()
    rgb, alpha, _ = scene.render_3dgs(w64, torch.tensor(Ks), W, H)
    ((rgb * v_rgb).sum() + alpha.sum()).backward()
    assert w64.grad.dtype == torch.float64 and w64.grad.device.type == "cpu"
    assert torch.equal(w64.grad, v_w.double().cpu())


def test_viewmat_bwd_is_deterministic(ctx):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("medium")   # 20 000 Gaussians: 79 blocks per camera
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(5))
    v_splats, a = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, None)
    b = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], dev(w2c), dev(Ks), info["_campos"], W, H,
                        info["_splats"], v_splats)
    torch.cuda.synchronize()
    assert float(a.abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_isolated_and_empty_cameras(ctx):
    g, w2c, Ks, W, H = make("small")
    # cotangents on camera 0 only: the other cameras' gradients are exactly zero
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(2))
    v_alpha = torch.randn(alpha.shape, device="cuda:0", generator=_gen(3))
    v_rgb[1:] = 0; v_alpha[1:] = 0
    _, vm = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha)
    assert float(vm[0].abs().max()) > 0
    assert float(vm[1:].abs().max()) == 0.0
    # a camera that looks away from every Gaussian (all its pairs culled) gets an exact zero
    w2c = w2c.copy()
    w2c[1] = synth.look_at_w2c((3.5, 0.0, 0.8), target=(10.0, 0.0, 0.8)).astype(np.float32)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    N = g["means"].shape[0]
    assert int((info["_splats"][N:2 * N, 10].view(torch.int32) > 0).sum()) == 0
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(4))
    _, vm = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, None)
    assert float(vm[0].abs().max()) > 0
    assert float(vm[1].abs().max()) == 0.0


def test_scene_c2w_gradient_through_two_renders(ctx):
    """Scene.w2c does not share one cached inverse between renders when c2w requires a gradient: two backward passes
    before an optimiser step both work, and c2w.grad is their sum chained through the inverse."""
    import starst3r_amd as st
    g, w2c, Ks, W, H = make("small")
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    scene.intrinsics = dev(Ks)
    c2w = torch.inverse(dev(w2c)).requires_grad_()
    scene.c2w = c2w
    v_rgb = torch.randn((w2c.shape[0], H, W, 3), device="cuda:0", generator=_gen(8))
    for _ in range(2):
        rgb, alpha, _ = scene.render_3dgs_original(W, H)
        ((rgb * v_rgb).sum() + alpha.sum()).backward()
    # the w2c gradient of the same render, then the float64 chain through inverse
    w = torch.inverse(c2w.detach()).requires_grad_()
    rgb, alpha, _ = scene.render_3dgs(w, scene.intrinsics, W, H)
    ((rgb * v_rgb).sum() + alpha.sum()).backward()
    c64 = c2w.detach().double().requires_grad_()
    (ref,) = torch.autograd.grad(torch.inverse(c64), c64, 2.0 * w.grad.double())
    err = rel_err_per_camera(c2w.grad, ref)
    print("c2w chain, max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    assert max(err) < 1e-6, err   # measured <= 7.6e-8
    with torch.no_grad():   # without grad mode the cached inverse is used as before
        assert scene.w2c is scene.w2c


def test_pose_recovery(ctx):
    """The capability itself: a perturbed camera is brought back by Adam on an se(3) correction through render_3dgs
    (L1 against images rendered at the true poses, Gaussians frozen)."""
    import starst3r_amd as st
    W, H = 160, 120
    g, w2c, Ks = synth.make_scene(20000, 3, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: dev(v) for k, v in g.items()}
    w_true = torch.tensor(w2c[1], dtype=torch.float64)
    K1 = dev(Ks[1:2])
    with torch.no_grad():
        gt, _, _ = scene.render_3dgs(dev(w2c[1:2]), K1, W, H)
    # perturb camera 1: 2 degrees about a random axis, 2 % of the baseline along a random direction
    rng = np.random.default_rng(5)
    axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
    dirn = rng.standard_normal(3); dirn /= np.linalg.norm(dirn)
    c0 = -w2c[0, :3, :3].T.astype(np.float64) @ w2c[0, :3, 3]; c1 = -w2c[1, :3, :3].T.astype(np.float64) @ w2c[1, :3, 3]
    baseline = float(np.linalg.norm(c1 - c0))
    rot = _se3_exp(torch.tensor(np.r_[axis * math.radians(2.0), 0, 0, 0]))
    w_pert = rot @ w_true
    R = w_pert[:3, :3]
    w_pert[:3, 3] = -R @ (-R.T @ w_pert[:3, 3] + torch.tensor(dirn * 0.02 * baseline))
    rot0, tr0 = _pose_errors(w_pert, w_true)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=2e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=200, eta_min=2e-4)
    for it in range(200):
        w = (_se3_exp(xi) @ w_pert)[None]
        rgb, _, _ = scene.render_3dgs(w, K1, W, H)
        loss = (rgb - gt).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step(); sched.step()
    rot1, tr1 = _pose_errors((_se3_exp(xi) @ w_pert).detach(), w_true)
    print("pose recovery: rotation %.2e -> %.2e rad, centre %.2e -> %.2e" % (rot0, rot1, tr0, tr1))
    # measured: centre 5.4e-2 -> 4.4e-5, rotation 3.5e-2 -> 7.5e-5 rad (about 1 s for the 200 iterations)
    assert rot1 < rot0 / 100 and tr1 < tr0 / 100, (rot0, rot1, tr0, tr1)


def test_full_size_one_view(ctx):
    """SYNTH-1M, one 1920x1080 view: ~3 900 blocks into the per-camera reduction.  The cotangents are not masked (the
    comparison is the kernel's chain rule on the HIP per-pair gradients, which the mask does not affect)."""
    W, H = 1920, 1080
    g, w2c, Ks = synth.make_scene(1_000_000, 1, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(6))
    v_alpha = torch.randn(alpha.shape, device="cuda:0", generator=_gen(7))
    v_splats, vm = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha)
    assert int((info["_splats"][:, 10].view(torch.int32) > 0).sum()) > 500_000
    ref = chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats)
    err = rel_err_per_camera(vm, ref)
    print("SYNTH-1M one view, max |d| / max |ref|:", ["%.1e" % e for e in err])
    assert max(err) < 1e-6, err   # measured 3.4e-8
