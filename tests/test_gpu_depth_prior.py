"""Training against depth maps: st3r_loss_depth_prior (loss_depth.hip), st3r_ctx_set_depth_prior inside the fused steps
(fused_step.hip) and run_3dgs_optim(depth_fac=...).

References: float64 torch for the loss kernel; for the fused gradient the unfused chain -- render_3dgs(..., "RGB+ED")
through autograd, ops.loss_l1_ssim, the depth term in torch -- and the float64 dense renderer of test_gpu_depth.py, which
measures that chain's own error; st3r_gs_train_step on a fresh context for everything that must not move.  Run on the
MI355X box:
    python -m pytest tests/test_gpu_depth_prior.py -m gpu -q -s
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as go
from st3r_synth import synth
from test_gpu_depth import render_dense_depth   # (the arithmetic dense_loss_grads restates band by band)
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _same_bits, _setup, _small_scene,
                            _synthetic_prior, dev, make, rel_err_per_camera)

BLOCKS = ("means", "quats", "scales", "opacities", "sh")
DEPTH_FAC = 0.5


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the loss kernel against float64 torch
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_inputs(C, H, W):
    gen = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    D = torch.rand((C, H, W, 1), generator=gen)
    alpha = 0.25 + 0.75 * torch.rand((C, H, W, 1), generator=gen)   # (ordinary pixels: ED = D / alpha <= 4)
    Z = 0.5 + torch.rand((C, H, W), generator=gen)
    w = torch.rand((C, H, W), generator=gen)
    w[torch.rand((C, H, W), generator=gen) < 0.3] = 0.0          # holes
    flat_a = alpha.view(-1)
    n = flat_a.numel()
    flat_a[::7] = 0.0                                             # alpha == 0 exactly
    flat_a[3::11] = 5e-11                                         # alpha in (0, 1e-10)
    # where alpha is clamped D is tiny too (a pixel nothing reached renders D = 0): ED = D / 1e-10 stays of order one, so the
    # sums are made of ordinary terms and atol = 1e-6 max(Z) n_c is the tolerance that binds
    flat_d = D.view(-1)
    flat_d[::7] *= 1e-10
    flat_d[3::11] *= 1e-10
    if n == 1:
        flat_a[0] = 0.37; flat_d[0] = 0.61
    if C > 1:
        w[C - 1] = 0.0                                            # one view without a single weight
    Z[w == 0] = float("nan")                                      # whatever the prior holds where w == 0
    if n > 4:
        Z.view(-1)[1] = float("inf"); w.view(-1)[1] = 0.0
    return D, alpha, Z, w


def _kernel_ref(D, alpha, Z, w, fac):
    D, alpha, Z, w = D.double()[..., 0], alpha.double()[..., 0], Z.double(), w.double()
    on = w > 0
    ac = alpha.clamp(min=1e-10)
    ed = D / ac
    diff = torch.where(on, ed - torch.where(on, Z, torch.zeros_like(Z)), torch.zeros_like(ed))
    s = (w * diff.abs()).sum((1, 2))
    n = w.sum((1, 2)).clamp(min=1.0)
    g = fac * w * torch.sign(diff) / n[:, None, None]
    v_d = g / ac
    v_a = torch.where(alpha >= 1e-10, -g * ed / ac, torch.zeros_like(g))
    return s, n, v_d, v_a


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 33), (3, 16, 64), (2, 37, 130)])
def test_loss_kernel_vs_fp64(ctx, shape):
    from starst3r_amd import ops
    C, H, W = shape
    D, alpha, Z, w = _kernel_inputs(C, H, W)
    s_ref, n_ref, vd_ref, va_ref = _kernel_ref(D, alpha, Z, w, DEPTH_FAC)
    args = [x.cuda().contiguous() for x in (D, alpha, Z, w)]
    sums, v_d, v_a = ops.loss_depth_prior(ctx, *args, DEPTH_FAC)
    sums2, v_d2, v_a2 = ops.loss_depth_prior(ctx, *args, DEPTH_FAC)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(v_d).all()) and bool(torch.isfinite(v_a).all())
    zmax = float(Z[w > 0].max()) if bool((w > 0).any()) else 1.0
    s, n = sums[:, 0].cpu(), sums[:, 1].cpu()
    # every term of the sums is ordinary (ED <= 4, Z <= 1.5), so a lost or mis-weighted pixel shows
    ed_all = (D.double() / alpha.double().clamp(min=1e-10))[..., 0]
    assert float(ed_all[w > 0].max() if bool((w > 0).any()) else 0.0) <= 4.0
    print(shape, "sums rel", float(((s - s_ref).abs() / s_ref.clamp(min=1e-300)).max()),
          "v_D rel", float(((v_d[..., 0].cpu().double() - vd_ref).abs() / vd_ref.abs().clamp(min=1e-300)).max()),
          "v_alpha rel", float(((v_a[..., 0].cpu().double() - va_ref).abs() / va_ref.abs().clamp(min=1e-300)).max()))
    # n_c: a sum of float32 weights in double
    np.testing.assert_allclose(n.numpy(), n_ref.numpy(), rtol=1e-12, atol=0)
    for c in range(C):
        np.testing.assert_allclose(float(s[c]), float(s_ref[c]), rtol=1e-6, atol=1e-6 * zmax * float(n_ref[c]))
    np.testing.assert_allclose(v_d[..., 0].cpu().double().numpy(), vd_ref.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(v_a[..., 0].cpu().double().numpy(), va_ref.numpy(), rtol=1e-6, atol=0)
    off = (w == 0)
    assert float(v_d[..., 0].cpu()[off].abs().max() if bool(off.any()) else 0.0) == 0.0
    assert float(v_a[..., 0].cpu()[off].abs().max() if bool(off.any()) else 0.0) == 0.0
    thin = (alpha[..., 0] < 1e-10)
    if bool(thin.any()):
        assert float(v_a[..., 0].cpu()[thin].abs().max()) == 0.0
    if C > 1:   # the view without weights: loss 0, n_c 1, gradients 0
        assert float(s[C - 1]) == 0.0 and float(n[C - 1]) == 1.0
        assert float(v_d[C - 1].abs().max()) == 0.0 and float(v_a[C - 1].abs().max()) == 0.0
    # the same inputs give the same bits
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    assert _same_bits(v_d, v_d2) and _same_bits(v_a, v_a2)


def test_loss_kernel_on_unaligned_buffers(ctx):
    """(3,16,64) has H * W a multiple of 4, but inputs that start 4 bytes past a 16-byte boundary take the 4-byte path: the
    gradients have the bits of the aligned call (the same float32 operations per pixel), n_c is equal (a sum of float32 in
    double: exact either way) and the sums stay within test_loss_kernel_vs_fp64's tolerance"""
    from starst3r_amd import ops
    C, H, W = 3, 16, 64
    D, alpha, Z, w = _kernel_inputs(C, H, W)
    s_ref, n_ref, _, _ = _kernel_ref(D, alpha, Z, w, DEPTH_FAC)

    def off(t):
        big = torch.zeros(t.numel() + 4, device="cuda:0")
        out = big[1:1 + t.numel()].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4
        return out
    sums, v_d, v_a = ops.loss_depth_prior(ctx, *[x.cuda().contiguous() for x in (D, alpha, Z, w)], DEPTH_FAC)
    sums_o, v_do, v_ao = ops.loss_depth_prior(ctx, *[off(x) for x in (D, alpha, Z, w)], DEPTH_FAC)
    torch.cuda.synchronize()
    assert _same_bits(v_do.clone(), v_d) and _same_bits(v_ao.clone(), v_a)
    assert torch.equal(sums_o[:, 1], sums[:, 1])
    np.testing.assert_allclose(sums_o[:, 1].cpu().numpy(), n_ref.numpy(), rtol=1e-12, atol=0)
    zmax = float(Z[w > 0].max())
    for c in range(C):
        np.testing.assert_allclose(float(sums_o[c, 0]), float(s_ref[c]), rtol=1e-6, atol=1e-6 * zmax * float(n_ref[c]))


@pytest.mark.parametrize("shape", [
    (1, 11, 11),     # odd H * W, one interior pixel
    (2, 12, 75),     # H * W a multiple of 4: the 16-byte path
    (2, 50, 37),     # H * W no multiple of 4: view 1 starts off a 16-byte boundary, the 4-byte path
    (1, 130, 70),    # several workgroups per view, a chunk edge (pixel 1024) inside a row
    (1, 10, 40),     # no interior: its sum is 0, max(., 1) gives 1
])
def test_both_losses_take_their_normalisers_from_one_weight_sum(ctx, shape):
    """st3r_loss_depth_prior's n_c (sums[:, 1]) and st3r_loss_l1_ssim_weighted's n1 (sums[:, 2]) come from one kernel
    (k_weight_sums, per_view.h): the same bits for the same map; its n2 (sums[:, 3]) is the same sum over the interior.
    The weights are multiples of 1/8 in [-1, 2] with a few NaNs: every double sum is exact in any order, so numpy's float64
    sum of the weights that count (w > 0; negative and NaN weights are 0) is compared with ==."""
    from starst3r_amd import ops
    C, H, W = shape
    rng = np.random.default_rng(100 * H + W)
    w = (rng.integers(-8, 17, (C, H, W)) / 8.0).astype(np.float32)
    w.reshape(-1)[rng.choice(w.size, max(2, w.size // 50), replace=False)] = np.nan
    if C > 1:
        w[C - 1] = np.minimum(w[C - 1], 0.0)     # a view in which nothing counts (NaNs stay): max(., 1) applies
    assert np.isnan(w).any() and (w[0] > 0).any() and (w < 0).any()
    counts = np.where(w > 0, w, np.float32(0)).astype(np.float64)
    n1_ref = np.maximum(counts.sum((1, 2)), 1.0)
    n2_ref = np.maximum(counts[:, 5:H - 5, 5:W - 5].sum((1, 2)), 1.0)
    img = lambda: torch.tensor(rng.random((C, H, W, 3), dtype=np.float32), device="cuda:0")
    plane = lambda lo: torch.tensor(lo + rng.random((C, H, W, 1), dtype=np.float32), device="cuda:0")
    wd = torch.tensor(w, device="cuda:0")
    dsums, _, _ = ops.loss_depth_prior(ctx, plane(0.0), plane(0.25), plane(0.5)[..., 0].contiguous(), wd, DEPTH_FAC)
    lsums, _ = ops.loss_l1_ssim_weighted(ctx, img(), img(), wd, 0.8, 0.2, want_grad=False)
    torch.cuda.synchronize()
    n_c, n1, n2 = dsums[:, 1].cpu(), lsums[:, 2].cpu(), lsums[:, 3].cpu()
    print(shape, "n_c", n_c.tolist(), "n1", n1.tolist(), "n2", n2.tolist(), "numpy", n1_ref.tolist(), n2_ref.tolist())
    assert torch.equal(n_c.view(torch.int64), n1.view(torch.int64))
    assert (n1.numpy() == n1_ref).all() and (n2.numpy() == n2_ref).all()
    if C > 1:
        assert float(n1[C - 1]) == 1.0 and float(n2[C - 1]) == 1.0
    if H <= 10:
        assert (n2.numpy() == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the fused-step tests
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().cpu().abs().max() + 1e-30))


def _depth_term(ed, Z, w, fac):
    n = w.sum((1, 2)).clamp(min=1.0)
    return fac * ((w * (ed - Z).abs()).sum((1, 2)) / n).sum()


def dense_loss_grads(g, w2c, Ks, W, H, rad, v_rgb, Z, wt, fac, tile_size=16):
    """Float64 gradients of  sum(rgb * v_rgb) + depth term  through test_gpu_depth.render_dense_depth's arithmetic, one block
    of 16 rows x 80 columns at a time: a block evaluates the Gaussians whose tile rectangle reaches it (every other one has alpha = 0
    there, a factor of exactly 1 in the products) and back-propagates at once, so memory and time follow the rectangles, not
    pixels x Gaussians (`wide`: 76800 pixels x 2500 Gaussians x 3 views).  The loss is a sum over pixels (n_c depends on the
    weights alone), so the bands' gradients add up.  -> dict of gradients (means, quats, scales, opacities, sh, w2c)"""
    import math
    from oracle import gs_torch_ref as tr
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    ref = {k: t(g[k]).requires_grad_() for k in ("means", "quats", "scales", "opacities", "shN")}
    vm = t(w2c).requires_grad_()
    K = t(Ks)
    v_rgb, Z, wt = t(v_rgb), t(Z), t(wt)
    n_c = wt.sum((1, 2)).clamp(min=1.0)
    tw, th = math.ceil(W / tile_size), math.ceil(H / tile_size)
    xs = torch.arange(W, dtype=torch.float64) + 0.5
    for c in range(w2c.shape[0]):
        idx = torch.nonzero(rad[c] > 0).reshape(-1)
        with torch.no_grad():
            m2, depth, _ = tr.project(ref["means"][idx], ref["quats"][idx], ref["scales"][idx], vm[c], K[c], W, H)
            order = torch.sort(depth.to(torch.float32), stable=True).indices
            idx = idx[order]; m2 = m2[order]
            r = rad[c][idx].to(torch.float64)
            x0 = torch.clamp(torch.floor((m2[:, 0] - r) / tile_size), 0, tw); x1 = torch.clamp(torch.ceil((m2[:, 0] + r) / tile_size), 0, tw)
            y0 = torch.clamp(torch.floor((m2[:, 1] - r) / tile_size), 0, th); y1 = torch.clamp(torch.ceil((m2[:, 1] + r) / tile_size), 0, th)
        for band, tb in ((b, k) for b in range(th) for k in range(0, tw, 5)):   # 16 rows x (up to) 5 tiles of columns
            sel = torch.nonzero((y0 <= band) & (band < y1) & (x0 < tb + 5) & (tb < x1)).reshape(-1)
            rows = torch.arange(band * tile_size, min((band + 1) * tile_size, H))
            cols = xs[tb * tile_size:min((tb + 5) * tile_size, W)]
            if sel.numel() == 0:
                continue
            ii = idx[sel]
            c2w = torch.inverse(vm)
            m, dep, conic = tr.project(ref["means"][ii], ref["quats"][ii], ref["scales"][ii], vm[c], K[c], W, H)
            col = tr.sh_color(ref["means"][ii], c2w[c, :3, 3], ref["shN"][ii])
            op = ref["opacities"][ii]
            px = cols.repeat(rows.numel()); py = (rows.to(torch.float64) + 0.5).repeat_interleave(cols.numel())
            cs = slice(int(cols[0]), int(cols[-1]) + 1)
            ptx = torch.div(px - 0.5, tile_size, rounding_mode="floor")
            in_rect = (ptx[:, None] >= x0[sel]) & (ptx[:, None] < x1[sel])
            dx = m[None, :, 0] - px[:, None]; dy = m[None, :, 1] - py[:, None]
            sigma = 0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) + conic[None, :, 1] * dx * dy
            alpha = torch.clamp_max(op[None] * torch.exp(-sigma), 0.999)
            valid = in_rect & (sigma >= 0) & (alpha >= 1.0 / 255.0)
            a = torch.where(valid, alpha, torch.zeros_like(alpha))
            stop = torch.cummax((torch.cumprod(1 - a, dim=1) <= 1e-4).to(torch.int8), dim=1).values.bool()
            a = torch.where(stop, torch.zeros_like(a), a)
            Tincl = torch.cumprod(1 - a, dim=1)
            Texcl = torch.cat([torch.ones_like(Tincl[:, :1]), Tincl[:, :-1]], dim=1)
            wgt = a * Texcl
            rgb = wgt @ col; acc = 1 - Tincl[:, -1]; d = (wgt @ dep[:, None])[:, 0]
            ed = d / acc.clamp(min=1e-10)
            sl = slice(int(rows[0]), int(rows[-1]) + 1)
            loss = (rgb * v_rgb[c, sl, cs].reshape(-1, 3)).sum() + \
                fac * (wt[c, sl, cs].reshape(-1) * (ed - Z[c, sl, cs].reshape(-1)).abs()).sum() / n_c[c]
            loss.backward()
    zero = lambda x, like: torch.zeros_like(like) if x is None else x
    out = {k: zero(ref[k].grad, ref[k]) for k in ("means", "quats", "scales", "opacities")}
    out["sh"] = zero(ref["shN"].grad, ref["shN"])[:, :4]
    out["w2c"] = zero(vm.grad, vm)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Per scene, computed once: the inputs of a step with a prior, the gradients of the unfused chain (float32, autograd
    through render_3dgs "RGB+ED"), those of the float64 dense renderer, and the unfused chain's error per block."""
    import starst3r_amd as st
    from starst3r_amd import ops
    ctx = ops.get_context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    Cn, N = w2c.shape[0], g["means"].shape[0]
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    _, _, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"], w2c, Ks, W, H,
                                  want_margin=True)
    Z, wt, _ = _synthetic_prior(ctx, P, vm, K, W, H, margin=meta["margin"])
    assert float(wt.sum()) > 0 and float((wt == 0).sum()) > 0
    # ---- the unfused chain
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(v.clone()) for k, v in P.items()}
    w = vm.clone().requires_grad_()
    img, alpha, _ = scene.render_3dgs(w, K, W, H, render_mode="RGB+ED")
    rgb, ed = img[..., :3], img[..., 3]
    csums, v_rgb = ops.loss_l1_ssim(ctx, rgb.detach().contiguous(), gt, 0.8, 0.2, want_grad=True)
    ((rgb * v_rgb).sum() + _depth_term(ed, Z, wt, DEPTH_FAC)).backward()
    info = ops.last_info()
    unf = {k: scene.gaussians[k].grad.clone() for k in ("means", "quats", "scales", "opacities")}
    unf["sh"] = scene.gaussians["shN"].grad[:, :4].clone()
    unf["w2c"] = w.grad.clone()
    # its loss, from the same kernels: colour sums + depth sums
    d = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha.detach(),
                            info["_last_ids"], Cn, W, H)
    dsums, v_d, v_a = ops.loss_depth_prior(ctx, d, alpha.detach().contiguous(), Z, wt, DEPTH_FAC)
    cnt = (H - 10) * (W - 10) * 3
    colour = float((0.8 * csums[:, 0] / (H * W * 3) + 0.2 * (1 - csums[:, 1] / cnt)).sum())
    loss = colour + float(DEPTH_FAC * (dsums[:, 0] / dsums[:, 1]).sum())
    # and with the depth term from torch, in double on the float32 ED of the unfused render
    loss_torch = colour + float(_depth_term(ed.detach().double(), Z.double(), wt.double(), DEPTH_FAC))
    # ---- the same chain from the stand-alone HIP entry points (the kernels the fused step runs): expected bit for bit
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    ops.blend_fwd(ctx, *lists, Cn, W, H)
    vs = ops.blend_bwd(ctx, *lists, alpha.detach(), info["_last_ids"], v_rgb, v_a, info["_cum_tiles"], Cn, W, H)
    vs.add_(ops.blend_depth_bwd(ctx, *lists, alpha.detach(), info["_last_ids"], v_d, info["_cum_tiles"], Cn, W, H))
    hip = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, info["_campos"],
                             W, H, info["_splats"], vs)
    hip_vm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H,
                             info["_splats"], vs)
    ops.depth_bwd(ctx, P["means"], vm, info["_splats"], vs, hip, hip_vm)
    # ---- float64 dense renderer
    rad = info["_splats"][:, 10].view(torch.int32).reshape(Cn, N).cpu().to(torch.int64)
    f64 = dense_loss_grads(g, w2c, Ks, W, H, rad, v_rgb.cpu(), Z.cpu(), wt.cpu(), DEPTH_FAC)
    err = {k: _rel(unf[k], f64[k]) for k in BLOCKS}
    err["w2c"] = rel_err_per_camera(unf["w2c"], f64["w2c"])
    torch.cuda.synchronize()
    return dict(P=P, vm=vm, K=K, campos=campos, gt=gt, Z=Z, wt=wt, W=W, H=H, unf=unf, f64=f64, err=err, loss=loss, loss_torch=loss_torch,
                hip=hip.clone(), hip_vm=hip_vm.clone(), offsets=info["isect_offsets"], n_isects=lists[2].numel())


def _fused_step(ctx, R, poses, debug=0, want_stats=True):
    """one fused step with the prior registered (learning rates 0: gradients and loss only) -> grads blocks, v_viewmats, loss"""
    from starst3r_amd import ops
    r = _Run(R["P"], R["vm"], R["campos"], 1)
    ops.set_depth_prior(ctx, R["gt"], R["Z"], R["wt"], DEPTH_FAC)
    ops.set_debug(ctx, debug)
    try:
        if poses:
            ops.train_step_poses(ctx, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.0, 0.0, r.grads, r.m,
                                 r.v, 0.0, B1, B2, EPS, 1, r.losses[0:1], r.pm, r.pv, 0.0, 1, None, r.vvm,
                                 want_stats=want_stats)
        else:
            ops.train_fwd_bwd(ctx, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.0, 0.0, r.grads,
                              r.losses[0:1], want_stats=want_stats)
    finally:
        ops.set_debug(ctx, 0)
        ops.set_depth_prior(ctx, None, None, None)
    torch.cuda.synchronize()
    return ops.split_grads(r.grads, R["P"]["means"].shape[0]), r.vvm, float(r.losses[0]), r.grads


def _check_against_reference(tag, R, G, vvm, loss):
    """the bar of the issue: per block, the fused step's error against the float64 dense renderer stays within twice the
    unfused chain's own; the loss is the colour loss plus the depth sums"""
    for k in BLOCKS:
        e = _rel(G[k], R["f64"][k])
        print(tag, k, "unfused %.2e fused %.2e vs float64" % (R["err"][k], e))
        assert e <= 2 * R["err"][k], (tag, k, e, R["err"][k])
    if vvm is not None:
        e = rel_err_per_camera(vvm, R["f64"]["w2c"])
        print(tag, "w2c per camera: unfused", ["%.1e" % x for x in R["err"]["w2c"]], "fused", ["%.1e" % x for x in e])
        for a, b in zip(e, R["err"]["w2c"]):
            assert a <= 2 * b, (tag, e, R["err"]["w2c"])
    # float32 store of a double sum whose terms carry test 1's 1e-6
    print(tag, "loss fused %.8f, colour loss + depth sums %.8f" % (loss, R["loss"]))
    assert abs(loss - R["loss"]) <= 2e-6 * abs(R["loss"]), (tag, loss, R["loss"])
    print(tag, "colour loss + torch's depth term %.8f" % R["loss_torch"])
    assert abs(loss - R["loss_torch"]) <= 2e-6 * abs(R["loss_torch"]), (tag, loss, R["loss_torch"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused gradient is the unfused chain's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_depth_gradient_equals_unfused_chain(name):
    from starst3r_amd import ops
    R = _reference(name)
    N = R["P"]["means"].shape[0]
    ctx = ops.Context("cuda:0")
    G, _, loss, flat = _fused_step(ctx, R, poses=False)
    _check_against_reference(name, R, G, None, loss)
    Gp, vvm, loss_p, flat_p = _fused_step(ctx, R, poses=True)
    _check_against_reference(name + " (poses)", R, Gp, vvm, loss_p)
    assert _same_bits(flat, flat_p) and loss == loss_p
    # this version materialises both per-pair arrays with the stand-alone kernels: the bits of the stand-alone chain
    assert _same_bits(flat, R["hip"]), name
    assert _same_bits(vvm, R["hip_vm"]), name
    for k in BLOCKS:
        print(name, k, "fused vs autograd chain: same bits" if _same_bits(G[k].contiguous(), R["unf"][k].contiguous())
              else "fused vs autograd chain: %.1e" % _rel(G[k], R["unf"][k]))
    # the prior does something: without it the gradient is another one
    r = _Run(R["P"], R["vm"], R["campos"], 1)
    ops.train_fwd_bwd(ctx, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.0, 0.0, r.grads, r.losses[0:1])
    torch.cuda.synchronize()
    assert not _same_bits(r.grads[:3 * N], flat[:3 * N]) and float(r.losses[0]) < loss
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. off means off
# ---------------------------------------------------------------------------------------------------------------------
def _two_train_steps(ctx, R, before=None):
    from starst3r_amd import ops
    if before is not None:
        before(ctx)
    ops.set_profiling(ctx, True)
    r = _Run(R["P"], R["vm"], R["campos"], 2)
    for it in range(2):
        ops.train_step(ctx, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3,
                       B1, B2, EPS, it + 1, r.losses[it:it + 1], want_stats=(it == 0))
        r.snaps.append(r.grads.clone())
    ops.settle(ctx)
    counts = {k: v[1] for k, v in ops.stage_ms(ctx).items()}
    ops.set_profiling(ctx, False)
    ops.set_depth_prior(ctx, None, None, None)
    # the counts are samples per stage and step (one per begin / end pair), not launches: a launch added inside a stage
    # would not show in them.  The arena does show the depth path: it allocates slots (depth, v_depth, v_alpha, the second
    # per-pair array, the loss partials) that no other path of the step touches.
    counts["arena_bytes"] = ctx.arena_bytes()
    return r, counts


def test_off_means_off():
    from starst3r_amd import ops
    R = _reference("small")

    def registered_then_cleared(ctx):
        ops.set_depth_prior(ctx, R["gt"], R["Z"], R["wt"], DEPTH_FAC)
        ops.set_depth_prior(ctx, None, None, None)

    def registered_with_zero(ctx):
        ops.set_depth_prior(ctx, R["gt"], R["Z"], R["wt"], 0.0)

    fresh_ctx = ops.Context("cuda:0")
    fresh, fresh_counts = _two_train_steps(fresh_ctx, R)
    fresh_ctx.close()
    assert sum(v for k, v in fresh_counts.items() if k != "arena_bytes") > 0
    for tag, before in (("no prior", None), ("cleared", registered_then_cleared), ("depth_fac == 0", registered_with_zero)):
        c = ops.Context("cuda:0")
        r, counts = _two_train_steps(c, R, before)
        c.close()
        assert counts == fresh_counts, (tag, counts, fresh_counts)
        for x, y in zip(r.state() + r.snaps, fresh.state() + fresh.snaps):
            assert _same_bits(x, y), tag
    # and on: the same two steps with the prior registered give other gradients
    c = ops.Context("cuda:0")
    r, on_counts = _two_train_steps(c, R, lambda cx: ops.set_depth_prior(cx, R["gt"], R["Z"], R["wt"], DEPTH_FAC))
    c.close()
    assert not _same_bits(r.snaps[0], fresh.snaps[0])
    assert on_counts["arena_bytes"] > fresh_counts["arena_bytes"]   # (off: not one of the depth path's slots exists)


# ---------------------------------------------------------------------------------------------------------------------
# 4. asynchronous equals synchronous; chunked views; the capacity / repeat protocol
# ---------------------------------------------------------------------------------------------------------------------
def _medium_with_prior(ctx, name="medium"):
    if name == "medium":
        P0, vm, K, campos, gt, W, H = _medium(ctx)
    else:
        g, w2c, Ks, W, H = make(name)
        P0, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Z, wt, info = _synthetic_prior(ctx, P0, vm, K, W, H)
    return P0, vm, K, campos, gt, W, H, Z, wt, info


def _step_poses_prior(ctx, r, K, gt, W, H, it, want_stats):
    from starst3r_amd import ops
    return ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2,
                                EPS, it + 1, r.losses[it:it + 1], r.pm, r.pv, 1e-3, it + 1, None, r.vvm,
                                want_stats=want_stats)


def test_async_depth_steps_equal_synchronous_steps():
    from starst3r_amd import ops
    steps = 5
    runs = []
    for want_stats in (True, False):
        ctx = ops.Context("cuda:0")   # a private context: the record-count hint is per context
        P0, vm, K, campos, gt, W, H, Z, wt, info = _medium_with_prior(ctx, "wide")
        # the scene has records in the last tile of the last camera: its end is the total the depth kernels must read
        # from the device in the asynchronous step
        assert int(info["isect_offsets"].reshape(-1)[-1]) < info["_flatten_ids_dense"].numel()
        ops.set_depth_prior(ctx, gt, Z, wt, DEPTH_FAC)
        r = _Run(P0, vm, campos, steps)
        for it in range(steps):
            _step_poses_prior(ctx, r, K, gt, W, H, it, want_stats)
        ops.settle(ctx)   # (no asynchronous step outgrew its buffers)
        torch.cuda.synchronize()
        runs.append(r)
        ctx.close()
    assert not _same_bits(runs[0].vm, vm)
    for x, y in zip(runs[0].state(), runs[1].state()):
        assert _same_bits(x, y)


def test_chunked_views_give_the_depth_gradient_of_the_whole_call():
    from starst3r_amd import ops
    R = _reference("many")   # 9 views: chunks of 4 and 5
    ctx = ops.Context("cuda:0")
    G, vvm, loss, _ = _fused_step(ctx, R, poses=True, debug=32)
    _check_against_reference("many, two view chunks", R, G, vvm, loss)
    ctx.close()


def test_chunked_depth_pose_step_has_the_bits_of_the_whole_call():
    """Depth prior + poses + two view chunks (debug flag 32) against the same step in one pass, bit for bit where the
    result is per view: a view belongs to one chunk, which runs the same kernels on that view's tiles, pairs and
    (camera, block) partials, so v_viewmats -- row 2 with the depth backward's addition included -- must not change.
    The loss is the float32 store of a double sum over the per-view sums, taken in view order either way; the per-view
    sums themselves are double accumulations whose order may depend on the launch (a relative 1e-15), so the two stores
    are the same float or neighbours: one float32 ulp, 2^-23 relative.  The parameter gradients of the chunked call are
    sums of chunk gradients (another association of the same float terms): printed, pinned by the test above."""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    N, V, W, H = 300, 3, 40, 24   # 3 x 2 tiles with ragged edges; chunks of 1 and 2 views
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=7, scale_lo=0.02, scale_hi=0.08)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Z, wt, _ = _synthetic_prior(ctx, P, vm, K, W, H)
    assert float(wt.sum()) > 0
    R = dict(P=P, vm=vm, K=K, campos=campos, gt=gt, Z=Z, wt=wt, W=W, H=H)
    _, vvm, loss, flat = _fused_step(ctx, R, poses=True)
    _, vvm_c, loss_c, flat_c = _fused_step(ctx, R, poses=True, debug=32)
    assert float(vvm.abs().max()) > 0 and float(vvm[:, 2].abs().max()) > 0
    print("chunked vs whole: loss %.9g %.9g, gradients %s" % (loss_c, loss, "same bits" if _same_bits(flat, flat_c)
          else "max rel %.1e" % _rel(flat_c, flat)))
    assert _same_bits(vvm, vvm_c), (vvm - vvm_c).abs().max()
    assert abs(loss_c - loss) <= 2.0 ** -23 * abs(loss), (loss_c, loss)
    ctx.close()


def test_overflowing_async_depth_step_moves_nothing_and_is_repeated():
    """debug flag 8 halves the capacity of an asynchronous step (the existing capacity mechanism): with a prior registered
    its records past the capacity are dropped in the depth kernels as in the colour kernels, neither update happens,
    st3r_ctx_settle reports it and the repeated step gives the undisturbed run, bit for bit."""
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        ctx = ops.Context("cuda:0")
        P0, vm, K, campos, gt, W, H, Z, wt, _ = _medium_with_prior(ctx)
        ops.set_depth_prior(ctx, gt, Z, wt, DEPTH_FAC)
        r = _Run(P0, vm, campos, 3)
        it = 0
        while it < 3:
            before = [x.clone() for x in r.state()[:-1]] if it == overflow_at else None
            if it == overflow_at:
                ops.set_debug(ctx, 8)
            _step_poses_prior(ctx, r, K, gt, W, H, it, want_stats=False)
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


# ---------------------------------------------------------------------------------------------------------------------
# 5. it helps
# ---------------------------------------------------------------------------------------------------------------------
HELP_ITERS = 100


@functools.lru_cache(maxsize=None)
def _help_scene():
    """20000 Gaussians, three 160 x 120 views; true images and true expected-depth maps from the true Gaussians; the start:
    every Gaussian moved along the ray of one camera (Gaussian i: camera i mod 3) by up to +-3 % of its distance"""
    from starst3r_amd import ops
    ctx = ops.get_context("cuda:0")
    W, H, V = 160, 120, 3
    g, w2c, Ks = synth.make_scene(20000, V, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    d = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                            info["_last_ids"], V, W, H)
    z_true = (d / alpha.clamp(min=1e-10))[..., 0].cpu()
    mask = (alpha[..., 0] > 0.5).cpu()
    rng = np.random.default_rng(23)
    centres = np.stack([-w2c[c, :3, :3].T @ w2c[c, :3, 3] for c in range(V)])
    own = centres[np.arange(g["means"].shape[0]) % V]
    start = {k: v.copy() for k, v in g.items()}
    start["means"] = (own + (g["means"] - own) * (1 + rng.uniform(-0.03, 0.03, (g["means"].shape[0], 1)))).astype(np.float32)
    return start, w2c, Ks, rgb.cpu().numpy(), z_true, mask, W, H


def _depth_error(scene, z_true, mask, W, H):
    with torch.no_grad():
        ed, _, _ = scene.render_3dgs_original(W, H, render_mode="ED")
    return float((ed[..., 0].cpu() - z_true).abs()[mask].mean())


@pytest.mark.parametrize("variant", ["plain", "poses", "pruning"])
def test_depth_prior_helps(ctx, variant):
    """The same HELP_ITERS iterations of run_3dgs_optim without and with the prior (depth_fac 1): the masked mean
    |ED - Z_true| of the original views.  Deterministic, so a fixed outcome.  Measured: 0.02562 at the start; plain 0.02013
    without / 0.00176 with the prior; pose_lr 1e-4 0.02034 / 0.00176; enable_pruning 0.02013 / 0.00176."""
    start, w2c, Ks, imgs, z_true, mask, W, H = _help_scene()
    kw = dict(plain={}, poses=dict(pose_lr=1e-4, pose_freeze=(0,)), pruning=dict(enable_pruning=True))[variant]
    out = {}
    for fac in (0.0, 1.0):
        scene = _optim_scene(start, torch.tensor(w2c), Ks, imgs)
        scene.depth_maps = [z_true[c] for c in range(z_true.shape[0])]
        scene.depth_confs = [torch.where(mask[c], 2.0, 0.0) for c in range(mask.shape[0])]   # confident where the truth is solid
        e0 = _depth_error(scene, z_true, mask, W, H)
        losses = scene.run_3dgs_optim(HELP_ITERS, depth_fac=fac, **kw)
        assert len(losses) == HELP_ITERS and all(np.isfinite(losses))
        out[fac] = _depth_error(scene, z_true, mask, W, H)
    print("depth prior, %s, %d iterations: masked mean |ED - Z_true| %.5f at the start, %.5f without, %.5f with the prior"
          % (variant, HELP_ITERS, e0, out[0.0], out[1.0]))
    assert out[1.0] < out[0.0] and out[1.0] < e0, (variant, e0, out)


# ---------------------------------------------------------------------------------------------------------------------
# 6. interface
# ---------------------------------------------------------------------------------------------------------------------
def test_add_images_keeps_the_depth_maps(monkeypatch):
    import starst3r_amd as st
    from starst3r_amd import scene as scene_mod
    from st3r_synth.synth_model import SyntheticPairwiseModel
    kept = {}
    real = scene_mod.reconstruct_scene

    def spy(*a, **k):
        kept["result"], params = real(*a, **k)
        return kept["result"], params
    monkeypatch.setattr(scene_mod, "reconstruct_scene", spy)
    scene = st.Scene(device="cuda:0")
    assert scene.depth_maps == [] and scene.depth_confs == []
    scene.add_images(SyntheticPairwiseModel(width=128, height=96, n_corr=300, seed=2), [torch.zeros(3, 96, 128)] * 2)
    res = kept["result"]
    pts, _, confs = res.get_dense_pts3d(clean_depth=True)
    z = res.get_dense_depth()
    assert len(scene.depth_maps) == 2 and len(scene.depth_confs) == 2
    for i in range(2):
        assert scene.depth_maps[i].shape == (96, 128) and scene.depth_maps[i].dtype == torch.float32
        assert scene.depth_confs[i].shape == (96, 128)
        assert torch.equal(scene.depth_maps[i], z[i].cpu()) and float(z[i].min()) > 0
        assert torch.equal(scene.depth_confs[i].reshape(-1), confs[i].reshape(-1).cpu().float())
        keep = (confs[i] > 1.5).reshape(-1).cpu()
        assert torch.equal(scene.dense_pts[i], pts[i].cpu()[keep])   # what add_images set before keeps its value
    # the maps are the depth of the dense points in their own camera
    w2c = scene.w2c.cpu()
    p = pts[0].cpu()
    zc = (p @ w2c[0, :3, :3].T + w2c[0, :3, 3])[:, 2].reshape(96, 128)
    np.testing.assert_allclose(zc.numpy(), scene.depth_maps[0].numpy(), rtol=1e-4, atol=1e-5)


def test_defaults_reach_the_loop_with_the_reference_arguments(monkeypatch):
    from starst3r_amd import scene as scene_mod
    scene, W, H = _small_scene()
    calls = []
    monkeypatch.setattr(scene_mod._gs, "run_3dgs_optim", lambda *a, **k: calls.append((a, k)) or [])
    scene.run_3dgs_optim(3)
    scene.run_3dgs_optim(3, depth_fac=0.0, depth_conf_thres=2.0)
    for a, k in calls:
        assert a == (scene, 3, False, 0.2, 0.01, 0.01, False) and k == {}
    scene.run_3dgs_optim(3, depth_fac=0.25)
    a, k = calls[-1]
    assert k["depth_fac"] == 0.25 and k["depth_conf_thres"] == 1.5


def test_missing_or_misshaped_maps_are_refused_before_anything_runs():
    scene, W, H = _small_scene()
    before = {k: v.detach().clone() for k, v in scene.gaussians.items()}
    maps = scene.depth_maps
    for bad in ([], maps[:-1], maps[:-1] + [torch.zeros(H, W + 1)]):
        scene.depth_maps = bad
        with pytest.raises(ValueError):
            scene.run_3dgs_optim(1, depth_fac=1.0)
    scene.depth_maps = maps
    scene.depth_confs = [torch.zeros(H + 1, W) for _ in maps]
    with pytest.raises(ValueError):
        scene.run_3dgs_optim(1, depth_fac=1.0)
    assert scene._gs_optim.step == 0 and all(torch.equal(before[k], scene.gaussians[k].detach()) for k in before)
    scene.depth_confs = []
    assert len(scene.run_3dgs_optim(2, depth_fac=1.0)) == 2   # all-ones weights


def test_depth_fac_under_the_gaussian_sharded_setting_is_refused(monkeypatch):
    scene, W, H = _small_scene()
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, depth_fac=1.0)
    assert scene._gs_optim.step == 0


def test_depth_fac_under_torch_distributed_is_refused(monkeypatch):
    from starst3r_amd import dist as sdist
    scene, W, H = _small_scene()
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        scene.run_3dgs_optim(1, depth_fac=1.0)
    assert scene._gs_optim.step == 0


def test_registration_is_cleared_when_the_loop_raises(monkeypatch):
    from starst3r_amd import gs as gs_mod, ops
    scene, W, H = _small_scene()
    ctx = ops.get_context("cuda:0")
    seen = []

    def boom(*a, **k):
        seen.append(ctx._dp_keep is not None)
        raise RuntimeError("stop")
    monkeypatch.setattr(gs_mod.ops, "train_step", boom)
    with pytest.raises(RuntimeError, match="stop"):
        scene.run_3dgs_optim(2, depth_fac=1.0)
    assert seen == [True] and ctx._dp_keep is None
    monkeypatch.undo()
    # the library forgot it too: a plain run equals one on a scene that never had a prior
    other, _, _ = _small_scene()
    scene._gs_optim.step = 0   # (the interrupted iteration had counted itself before it raised; nothing was updated)
    a = scene.run_3dgs_optim(2)
    b = other.run_3dgs_optim(2)
    assert a == b
