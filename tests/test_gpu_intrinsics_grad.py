"""Intrinsics gradients: st3r_gs_intrinsics_bwd (gs_intrinsics.hip) and render_3dgs with scene.intrinsics_grad
back-propagating into the intrinsics (gsplat returns no such gradient; it is opt-in here).

The references are float64 torch autograd with respect to K: through oracle/gs_torch_ref's projection for the kernel in
isolation, through its dense renderer end to end.  Errors are per camera, max |d| / max |ref| on the scaled vector
(fx v_fx, fy v_fy, W v_cx, H v_cy), whose four entries share a unit.  Run on the MI355X box:
    python -m pytest tests/test_gpu_intrinsics_grad.py -m gpu -q -s
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as go
from oracle import gs_torch_ref as tr
from st3r_synth import synth
from per_view_cases import _gen, dev, make, masked_cotangents, rel_err_per_camera, run_hip


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def clamp_scene():
    """One camera at the origin with an off-centre principal point and fx != fy.  Gaussians 0-3: the projected mean lies
    beyond the limit x high (1.15 W - cx), x low (-(0.15 W + cx)), y high (1.15 H - cy), y low (-(0.15 H + cy)) -- in
    that order -- while their radius (40 .. 54 pixels) still reaches into the image; Gaussians 4-7: small and inside."""
    W, H = 96, 64
    Ks = np.array([[[80.0, 0, 50.0], [0, 76.0, 30.0], [0, 0, 1]]], np.float32)
    w2c = np.eye(4, dtype=np.float32)[None]
    means = np.array([[1.7, 0.1, 2.0], [-1.8, -0.1, 2.0], [0.1, 1.3, 2.0], [-0.1, -1.25, 2.0],
                      [0.2, 0.1, 2.5], [-0.4, 0.2, 3.0], [0.3, -0.3, 2.2], [-0.2, -0.1, 2.8]], np.float32)
    scales = np.array([[0.30, 0.25, 0.35]] * 4 + [[0.06, 0.09, 0.05]] * 4, np.float32)
    rng = np.random.default_rng(4)
    q = rng.standard_normal((8, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    sh = np.zeros((8, 24, 3), np.float32); sh[:, :4] = rng.uniform(-0.5, 0.5, (8, 4, 3))
    g = dict(means=means, scales=scales, quats=q.astype(np.float32), opacities=np.full(8, 0.9, np.float32),
             sh0=np.zeros((8, 1, 3), np.float32), shN=sh)
    return g, w2c, Ks, W, H


def pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha):
    """HIP v_splats of the rasterization, then the kernel under test"""
    from starst3r_amd import ops
    Cn = w2c.shape[0]
    v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                             info["_last_ids"], v_rgb, v_alpha, info["_cum_tiles"], Cn, W, H)
    vk = ops.intrinsics_bwd(ctx, P["means"], P["quats"], P["scales"], dev(w2c), dev(Ks), W, H, info["_splats"], v_splats)
    torch.cuda.synchronize()
    return v_splats, vk


def k4(gK):
    """[C,3,3] gradient of K -> [C,4]: fx, fy, cx, cy"""
    return torch.stack([gK[:, 0, 0], gK[:, 1, 1], gK[:, 0, 2], gK[:, 1, 2]], dim=-1)


def chain_ref(g, w2c, Ks, W, H, splats, v_splats):
    """float64 autograd of (means2d, conic) of the visible pairs into K, with the HIP per-pair gradients as cotangents
    (the colour does not depend on K); vectorised over each camera's pairs.  -> [C,4]"""
    N, Cn = g["means"].shape[0], w2c.shape[0]
    rad = splats[:, 10].view(torch.int32).reshape(Cn, N).cpu()
    vs = v_splats.reshape(Cn, N, 12).double().cpu()
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    means, quats, scales = t(g["means"]), t(g["quats"]), t(g["scales"])
    vm = t(w2c)
    K = t(Ks).requires_grad_()
    outs, cots = [], []
    for c in range(Cn):
        idx = torch.nonzero(rad[c] > 0).reshape(-1)
        if idx.numel() == 0:
            continue
        m2, _, conic = tr.project(means[idx], quats[idx], scales[idx], vm[c], K[c], W, H)
        outs += [m2, conic]
        cots += [vs[c, idx, 0:2], vs[c, idx, 3:6]]
    if not outs:
        return torch.zeros((Cn, 4), dtype=torch.float64)
    (gk,) = torch.autograd.grad(outs, K, cots)
    assert float(gk[:, 2].abs().max()) == 0.0 and float(gk[:, 0, 1].abs().max()) == 0.0 and float(gk[:, 1, 0].abs().max()) == 0.0
    return k4(gk)


def scaled(v4, Ks, W, H):
    """(fx v_fx, fy v_fy, W v_cx, H v_cy): the gradient with respect to (log fx, log fy, cx / W, cy / H)"""
    K = torch.as_tensor(Ks).double().cpu()
    s = torch.stack([K[:, 0, 0], K[:, 1, 1], torch.full_like(K[:, 0, 0], float(W)), torch.full_like(K[:, 0, 0], float(H))], -1)
    return v4.detach().double().cpu() * s


FUZZ3 = ["fuzz0", "fuzz1", "fuzz2"]
# float32 per-pair arithmetic against float64: about a decade above what was measured (see the assertions)
TOL_REGULAR, TOL_FUZZ, TOL_END_TO_END = 1e-6, 1e-3, 3e-4


@pytest.mark.parametrize("name", ["small", "ragged", "one", "many", "wide", "n256", "n257"] + FUZZ3)
def test_kernel_vs_fp64_chain_rule(ctx, name):
    g, w2c, Ks, W, H = make(name)
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_splats, vk = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, dev(v_rgb), dev(v_alpha))
    assert tuple(vk.shape) == (w2c.shape[0], 4)
    ref = scaled(chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats), Ks, W, H)
    assert float(ref.abs().max()) > 0
    err = rel_err_per_camera(scaled(vk, Ks, W, H), ref)
    print(name, "max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    # measured: regular scenes <= 8.7e-8 (n256), fuzz scenes <= 7.2e-5 (fuzz2; Gaussians right in front of the camera,
    # whose 1/z^2 terms the float32 per-pair arithmetic carries); the bars are about a decade above
    tol = TOL_FUZZ if name.startswith("fuzz") else TOL_REGULAR
    assert max(err) < tol, (name, err)


def test_finisher_takes_a_second_trip(ctx):
    """65 792 Gaussians = 257 blocks of 256 for one camera: the finishing workgroup's strided loop over the partials runs
    twice for thread 0.  The cotangents are not masked (the comparison is the kernel's chain rule on the HIP per-pair
    gradients, which the mask does not affect)."""
    N, W, H = 256 * 257, 48, 32
    g, w2c, Ks = synth.make_scene(N, 1, W, H, seed=41, scale_lo=0.004, scale_hi=0.03)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(6))
    v_alpha = torch.randn(alpha.shape, device="cuda:0", generator=_gen(7))
    v_splats, vk = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha)
    rad = info["_splats"][:, 10].view(torch.int32)
    assert int((rad[256 * 256:] > 0).sum()) > 0   # the last block contributes
    ref = scaled(chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats), Ks, W, H)
    err = rel_err_per_camera(scaled(vk, Ks, W, H), ref)
    print("257 blocks, max |d| / max |ref|:", ["%.1e" % e for e in err])
    assert max(err) < TOL_REGULAR, err   # measured 2.0e-8


def test_clamped_pairs(ctx):
    """the four branches in which the clamp limit, and through it K, decides the Jacobian's third column"""
    g, w2c, Ks, W, H = clamp_scene()
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_splats, vk = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, dev(v_rgb), dev(v_alpha))
    # from the records: all eight are visible, and every one of them receives a gradient
    assert bool((info["_splats"][:, 10].view(torch.int32) > 0).all())
    assert bool((v_splats.reshape(8, 12)[:, 3:6].abs().max(dim=1).values > 0).all())
    # from the float64 side: Gaussians 0-3 are clamped, each at its own limit, and 4-7 are not
    fx, fy, cx, cy = (float(Ks[0, 0, 0]), float(Ks[0, 1, 1]), float(Ks[0, 0, 2]), float(Ks[0, 1, 2]))
    m = g["means"].astype(np.float64)
    u, v = fx * m[:, 0] / m[:, 2], fy * m[:, 1] / m[:, 2]   # mean2d - (cx, cy); the camera is the identity
    x_hi, x_lo, y_hi, y_lo = u > 1.15 * W - cx, u < -(0.15 * W + cx), v > 1.15 * H - cy, v < -(0.15 * H + cy)
    assert x_hi.tolist() == [True] + [False] * 7 and x_lo.tolist() == [False, True] + [False] * 6
    assert y_hi.tolist() == [False, False, True] + [False] * 5 and y_lo.tolist() == [False] * 3 + [True] + [False] * 4
    ref = scaled(chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats), Ks, W, H)
    err = rel_err_per_camera(scaled(vk, Ks, W, H), ref)
    print("clamped pairs, max |d| / max |ref|:", ["%.1e" % e for e in err], "ref", ref.tolist())
    assert max(err) < TOL_REGULAR, err   # measured 3.8e-8
    # the clamp terms matter: without dcj/dcx = 1/z the principal-point gradient is another one
    plain = v_splats.reshape(8, 12)[:, 0:2].double().sum(0).cpu() * torch.tensor([float(W), float(H)], dtype=torch.float64)
    assert float((plain - ref[0, 2:]).abs().max() / ref[0].abs().max()) > 1e-3


def render_dense_depth(means, quats, scales, opacities, sh, viewmats, Ks, W, H, vis_mask, radii, tile_size=16):
    """gs_torch_ref.render_dense with one more output: depth [C,H,W,1] = sum_i w_i z_i, the same weights (as
    tests/test_gpu_depth.py)"""
    Cn = viewmats.shape[0]
    dt = means.dtype
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt) + 0.5, torch.arange(W, dtype=dt) + 0.5, indexing="ij")
    px = xs.reshape(-1); py = ys.reshape(-1)
    ptx = torch.div(px - 0.5, tile_size, rounding_mode="floor"); pty = torch.div(py - 0.5, tile_size, rounding_mode="floor")
    tw = math.ceil(W / tile_size); th = math.ceil(H / tile_size)
    out_rgb, out_a, out_d = [], [], []
    c2w = torch.inverse(viewmats)
    for c in range(Cn):
        idx = torch.nonzero(vis_mask[c]).reshape(-1)
        m2, depth, conic = tr.project(means[idx], quats[idx], scales[idx], viewmats[c], Ks[c], W, H)
        col = tr.sh_color(means[idx], c2w[c, :3, 3], sh[idx])
        op = opacities[idx]
        order = torch.sort(depth.detach().to(torch.float32), stable=True).indices
        m2, conic, col, op, depth = m2[order], conic[order], col[order], op[order], depth[order]
        rad = radii[c][idx][order].to(dt)
        m2d = m2.detach()
        x0 = torch.clamp(torch.floor((m2d[:, 0] - rad) / tile_size), 0, tw)
        x1 = torch.clamp(torch.ceil((m2d[:, 0] + rad) / tile_size), 0, tw)
        y0 = torch.clamp(torch.floor((m2d[:, 1] - rad) / tile_size), 0, th)
        y1 = torch.clamp(torch.ceil((m2d[:, 1] + rad) / tile_size), 0, th)
        in_rect = (ptx[:, None] >= x0) & (ptx[:, None] < x1) & (pty[:, None] >= y0) & (pty[:, None] < y1)
        dx = m2[None, :, 0] - px[:, None]; dy = m2[None, :, 1] - py[:, None]
        sigma = 0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) + conic[None, :, 1] * dx * dy
        alpha = torch.clamp_max(op[None] * torch.exp(-sigma), 0.999)
        valid = in_rect & (sigma >= 0) & (alpha >= 1.0 / 255.0)
        a = torch.where(valid, alpha, torch.zeros_like(alpha))
        stop = torch.cummax((torch.cumprod(1 - a, dim=1) <= 1e-4).to(torch.int8), dim=1).values.bool()
        a = torch.where(stop, torch.zeros_like(a), a)
        Tincl = torch.cumprod(1 - a, dim=1)
        Texcl = torch.cat([torch.ones_like(Tincl[:, :1]), Tincl[:, :-1]], dim=1)
        w = a * Texcl
        Tfin = Tincl[:, -1] if Tincl.shape[1] else torch.ones_like(px)
        out_rgb.append((w @ col).reshape(H, W, 3)); out_a.append((1 - Tfin).reshape(H, W, 1))
        out_d.append((w @ depth[:, None]).reshape(H, W, 1))
    return torch.stack(out_rgb), torch.stack(out_a), torch.stack(out_d)


def _scene(g):
    import starst3r_amd as st
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    return scene


@pytest.mark.parametrize("mode", ["RGB", "RGB+ED"])
@pytest.mark.parametrize("name", ["small", "ragged", "one", "many"])
def test_render_intrinsics_grad_vs_dense_fp64(ctx, name, mode):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    Cn, N = w2c.shape[0], g["means"].shape[0]
    _, alpha_o, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"], w2c, Ks, W, H,
                                        want_margin=True)
    ch = 4 if mode == "RGB+ED" else 3
    rng = np.random.default_rng(11)
    v_img = rng.standard_normal((Cn, H, W, ch)).astype(np.float32)
    v_alpha = rng.standard_normal(alpha_o.shape).astype(np.float32)
    und = ~(meta["margin"] > 1e-4)
    v_img[und] = 0.0; v_alpha[und] = 0.0
    if mode == "RGB+ED":
        # the quotient amplifies float32 noise where alpha is small: cotangents of ED only where alpha > 0.05
        v_img[..., -1][~(alpha_o[..., 0] > 0.05)] = 0.0
        assert min(float((v_img[c, ..., -1] != 0).mean()) for c in range(Cn)) > 0
    scene = _scene(g)
    scene.intrinsics_grad = True
    K = dev(Ks).requires_grad_()
    img, alpha, _ = scene.render_3dgs(dev(w2c), K, W, H, render_mode=mode)
    ((img * dev(v_img)).sum() + (alpha * dev(v_alpha)).sum()).backward()
    assert tuple(K.grad.shape) == (Cn, 3, 3)
    zero = torch.ones((3, 3), dtype=torch.bool); zero[0, 0] = zero[1, 1] = zero[0, 2] = zero[1, 2] = False
    assert float(K.grad.cpu()[:, zero].abs().max()) == 0.0   # skew and row 2 get none
    info = ops.last_info()
    rad = info["_splats"][:, 10].view(torch.int32).reshape(Cn, N).cpu().to(torch.int64)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    K64 = t(Ks).requires_grad_()
    rgb_t, alpha_t, d_t = render_dense_depth(t(g["means"]), t(g["quats"]), t(g["scales"]), t(g["opacities"]), t(g["shN"]),
                                             t(w2c), K64, W, H, rad > 0, rad)
    img_t = torch.cat([rgb_t, d_t / alpha_t.clamp(min=1e-10)], dim=-1) if mode == "RGB+ED" else rgb_t
    ((img_t * t(v_img)).sum() + (alpha_t * t(v_alpha)).sum()).backward()
    ref = scaled(k4(K64.grad), Ks, W, H)
    assert float(ref.abs().max()) > 0
    err = rel_err_per_camera(scaled(k4(K.grad), Ks, W, H), ref)
    print(name, mode, "end to end, max |d| / max |ref| per camera:", ["%.1e" % e for e in err])
    assert max(err) <= TOL_END_TO_END, (name, mode, err)   # measured <= 1.9e-5 ("RGB", ragged), <= 2.9e-5 ("RGB+ED", ragged)


def test_intrinsics_gradient_is_opt_in_and_changes_nothing_else(ctx):
    g, w2c, Ks, W, H = make("small")
    scene = _scene(g)
    v_rgb = torch.randn((w2c.shape[0], H, W, 3), device="cuda:0", generator=_gen(1))
    grads = []
    for k_grad in (False, True):
        for p in scene.gaussians.values():
            p.grad = None
        w = dev(w2c).requires_grad_()
        K = dev(Ks).requires_grad_()
        scene.intrinsics_grad = k_grad
        rgb, alpha, _ = scene.render_3dgs(w, K, W, H)
        ((rgb * v_rgb).sum() + alpha.sum()).backward()
        assert (K.grad is not None) == k_grad
        out = {k: p.grad.clone() for k, p in scene.gaussians.items() if p.grad is not None}
        out["w2c"] = w.grad.clone()
        grads.append(out)
        if k_grad:
            assert float(K.grad.abs().max()) > 0
            v_K = K.grad.clone()
    assert grads[0].keys() == grads[1].keys() and "means" in grads[0]
    for k in grads[0]:
        assert torch.equal(grads[0][k].view(torch.int32), grads[1][k].view(torch.int32)), k
    # intrinsics that require no gradient get none, asked for or not
    rgb, alpha, _ = scene.render_3dgs(dev(w2c), dev(Ks), W, H)
    (rgb * v_rgb).sum().backward()
    # float64 CPU intrinsics get their gradient back in their own dtype and device (autograd through render_3dgs' .to())
    K64 = torch.tensor(Ks, dtype=torch.float64).requires_grad_()
    rgb, alpha, _ = scene.render_3dgs(dev(w2c), K64, W, H)
    ((rgb * v_rgb).sum() + alpha.sum()).backward()
    assert K64.grad.dtype == torch.float64 and K64.grad.device.type == "cpu"
    assert torch.equal(K64.grad, v_K.double().cpu())


def test_intrinsics_bwd_is_deterministic(ctx):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("medium")   # 20 000 Gaussians: 79 blocks per camera
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(5))
    v_splats, a = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, None)
    b = ops.intrinsics_bwd(ctx, P["means"], P["quats"], P["scales"], dev(w2c), dev(Ks), W, H, info["_splats"], v_splats)
    torch.cuda.synchronize()
    assert float(a.abs().min()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_isolated_and_empty_cameras(ctx):
    g, w2c, Ks, W, H = make("small")
    # cotangents on camera 0 only: the other cameras' gradients are exactly zero
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(2))
    v_alpha = torch.randn(alpha.shape, device="cuda:0", generator=_gen(3))
    v_rgb[1:] = 0; v_alpha[1:] = 0
    _, vk = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, v_alpha)
    assert float(vk[0].abs().max()) > 0
    assert float(vk[1:].abs().max()) == 0.0
    # a camera that looks away from every Gaussian (all its pairs culled) gets an exact zero
    w2c = w2c.copy()
    w2c[1] = synth.look_at_w2c((3.5, 0.0, 0.8), target=(10.0, 0.0, 0.8)).astype(np.float32)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    N = g["means"].shape[0]
    assert int((info["_splats"][N:2 * N, 10].view(torch.int32) > 0).sum()) == 0
    v_rgb = torch.randn(rgb.shape, device="cuda:0", generator=_gen(4))
    _, vk = pair_grads(ctx, P, rgb, alpha, info, w2c, Ks, W, H, v_rgb, None)
    assert float(vk[0].abs().max()) > 0
    assert float(vk[1].abs().max()) == 0.0


def test_focal_recovery(ctx):
    """The capability itself: one view, Gaussians and pose frozen, the ground truth rendered at the true K; fx = fy start
    5 % off and torch Adam on log f through render_3dgs (scene.intrinsics_grad) brings them back.  A condition, not a
    measurement: the problem is well-posed, the focal error must fall at least tenfold within 300 iterations."""
    W, H = 160, 120
    g, w2c, Ks = synth.make_scene(20000, 3, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    scene = _scene(g)
    scene.gaussians = {k: dev(v) for k, v in g.items()}
    scene.intrinsics_grad = True
    w = dev(w2c[1:2])
    K_true = torch.tensor(Ks[1], dtype=torch.float64)
    with torch.no_grad():
        gt, _, _ = scene.render_3dgs(w, dev(Ks[1:2]), W, H)
    f0 = 1.05 * float(K_true[0, 0])
    logf = torch.tensor(math.log(f0), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([logf], lr=5e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=300, eta_min=1e-4)

    def K_of(lf):
        f = torch.exp(lf)
        z, o = torch.zeros_like(f), torch.ones_like(f)
        return torch.stack([torch.stack([f, z, K_true[0, 2] * o]), torch.stack([z, f, K_true[1, 2] * o]),
                            torch.stack([z, z, o])])[None]

    for it in range(300):
        rgb, _, _ = scene.render_3dgs(w, K_of(logf), W, H)
        loss = (rgb - gt).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step(); sched.step()
    e0 = abs(f0 / float(K_true[0, 0]) - 1.0)
    e1 = abs(float(torch.exp(logf.detach())) / float(K_true[0, 0]) - 1.0)
    print("focal recovery: relative focal error %.2e -> %.2e (%.0fx)" % (e0, e1, e0 / max(e1, 1e-30)))
    # measured 5.00e-2 -> 1.82e-6 (about 1 s for the 300 iterations)
    assert e1 <= e0 / 10, (e0, e1)
