"""GPU tests of the per-pixel loss weights: the weighted loss kernels (csrc/loss.hip, WGT instantiations of k_ssim_fwd and of
k_ssim_fused in both of its forms) through st3r_loss_l1_ssim_weighted, the registration st3r_ctx_set_loss_weight in the fused
training calls, and scene.loss_masks through run_3dgs_optim.

    1. against the float64 reference of tests/loss_mask_cases.py      4. the fused step equals the unfused chain
    2. all ones is the unweighted kernel, bit for bit                 5. nothing else moves
    3. zero weight means zero influence                               6. through run_3dgs_optim

The shapes of 1 - 3 are those of tests/test_gpu_loss.py (every one has ceil(W / 64) * C <= 6, so the row bands are
max(1, H // 64) under the 512-slot rule of the weighted kernels as under the others)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_adam_cases as lac
import loss_mask_cases as lmc
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _same_bits, _setup, _synthetic_prior, dev, make)
from st3r_synth import synth
from test_gpu_loss import SHAPES

KERNELS = ("k_ssim_fwd<wgt>", "k_ssim_fused<false,wgt>", "k_ssim_fused<true,wgt>")
BUILDERS = sorted(lmc.WEIGHTS)
DEPTH_FAC = 0.5


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def _ids(s):
    return "x".join(map(str, s))


def _img_seed(H, W, c):
    return 1000 * H + W + 17 * c      # test_gpu_loss.case's


@functools.lru_cache(maxsize=None)
def images(shape, content):
    Cn, H, W = shape
    xs, ys = zip(*(lac.BUILDERS[content](H, W, _img_seed(H, W, c)) for c in range(Cn)))
    x, y = np.stack(xs), np.stack(ys)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def case(shape, content, builder):
    """images, weights, the float64 reference per view and the gradient bounds per view; computed once, modified by nobody"""
    Cn, H, W = shape
    x, y = images(shape, content)
    w_seed = 31 * H + W
    w = lmc.weights_for(builder, Cn, H, W, w_seed)
    w.setflags(write=False)
    refs = [lmc.weighted_loss_grad(x[c], y[c], w[c]) for c in range(Cn)]
    bounds = []
    for c in range(Cn):
        e_max, e_elem = lmc.float32_reference_error(content, H, W, _img_seed(H, W, c), builder, Cn, c, w_seed)
        bounds.append((max(2e-6, 4 * e_max), max(1e-5, 4 * e_elem)))
    return x, y, w, refs, bounds


def run_weighted(ctx, X, Y, Wt):
    """kernel name -> (sums [C,4], v_render or None) as numpy"""
    from starst3r_amd import ops
    out = {}
    ops.set_gt_moments(ctx, None, None)
    out[KERNELS[0]] = ops.loss_l1_ssim_weighted(ctx, X, Y, Wt, lac.W_L1, lac.W_SSIM, want_grad=False)
    out[KERNELS[1]] = ops.loss_l1_ssim_weighted(ctx, X, Y, Wt, lac.W_L1, lac.W_SSIM)
    ops.set_gt_moments(ctx, Y, ops.gt_moments(ctx, Y))
    try:
        out[KERNELS[2]] = ops.loss_l1_ssim_weighted(ctx, X, Y, Wt, lac.W_L1, lac.W_SSIM)
        torch.cuda.synchronize()
    finally:
        ops.set_gt_moments(ctx, None, None)
    assert out[KERNELS[0]][1] is None
    return {k: (s.cpu().numpy(), None if v is None else v.cpu().numpy()) for k, (s, v) in out.items()}


def run_unweighted(ctx, X, Y):
    from starst3r_amd import ops
    out = {}
    ops.set_gt_moments(ctx, None, None)
    out[KERNELS[0]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM, want_grad=False)
    out[KERNELS[1]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
    ops.set_gt_moments(ctx, Y, ops.gt_moments(ctx, Y))
    try:
        out[KERNELS[2]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
        torch.cuda.synchronize()
    finally:
        ops.set_gt_moments(ctx, None, None)
    return {k: (s.cpu().numpy(), None if v is None else v.cpu().numpy()) for k, (s, v) in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_weighted_kernels_vs_float64_reference(ctx, shape, content, builder):
    Cn, H, W = shape
    x, y, w, refs, bounds = case(shape, content, builder)
    res = run_weighted(ctx, dev(x), dev(y), dev(w))
    tag = f"{Cn}x{H}x{W} {content} {builder}"
    fails = []
    for kernel in KERNELS:
        sums, v = res[kernel]
        worst = dict(l1=0.0, ssim=0.0, gmax=0.0, gelem=0.0)
        for c in range(Cn):
            r = refs[c]
            # the normalisers: sums of float32 weights in double, exact to rounding
            assert abs(sums[c, 2] - r["n1"]) <= 1e-12 * r["n1"] and abs(sums[c, 3] - r["n2"]) <= 1e-12 * r["n2"], \
                (tag, kernel, c, sums[c], r["n1"], r["n2"])
            e_l1 = abs(sums[c, 0] / (3 * sums[c, 2]) - r["l1"])
            e_ss = abs(sums[c, 1] / (3 * sums[c, 3]) - r["ssim"])
            if not (H > 10 and W > 10):
                assert sums[c, 1] == 0.0, (tag, kernel, c, "SSIM sum of an image without interior")
            worst["l1"] = max(worst["l1"], e_l1); worst["ssim"] = max(worst["ssim"], e_ss)
            if e_l1 >= 1e-6: fails.append((kernel, c, "weighted mean L1", e_l1, 1e-6))
            if e_ss >= 1e-5: fails.append((kernel, c, "weighted mean SSIM", e_ss, 1e-5))
            if v is not None:
                assert np.isfinite(v[c]).all(), (tag, kernel, c)
                g_max, g_elem = lmc.grad_errors(v[c], r["grad"])
                worst["gmax"] = max(worst["gmax"], g_max); worst["gelem"] = max(worst["gelem"], g_elem)
                if g_max > bounds[c][0]: fails.append((kernel, c, "gradient of max", g_max, bounds[c][0]))
                if g_elem > bounds[c][1]: fails.append((kernel, c, "gradient element-wise", g_elem, bounds[c][1]))
        b = (max(b[0] for b in bounds), max(b[1] for b in bounds))
        print(f"WLOSS {tag} {kernel}: L1 {worst['l1']:.2e} (1e-6) SSIM {worst['ssim']:.2e} (1e-5)"
              + ("" if v is None else f" grad/max {worst['gmax']:.2e} ({b[0]:.2e}) grad/elem {worst['gelem']:.2e} ({b[1]:.2e})"))
    assert not fails, (tag, fails)
    # the two fused forms take the ground truth's taps in the same order: the same gradient bits
    assert np.array_equal(res[KERNELS[1]][1].view(np.int32), res[KERNELS[2]][1].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. all ones is the unweighted kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_all_ones_give_the_bits_of_the_unweighted_kernels(ctx, shape, content):
    Cn, H, W = shape
    x, y = images(shape, content)
    X, Y = dev(x), dev(y)
    wgt = run_weighted(ctx, X, Y, torch.ones((Cn, H, W), device="cuda:0"))
    ref = run_unweighted(ctx, X, Y)
    for kernel in KERNELS:
        sums, v = wgt[kernel]
        assert np.array_equal(sums[:, :2].view(np.int64), ref[kernel][0].view(np.int64)), (kernel, sums, ref[kernel][0])
        assert np.all(sums[:, 2] == H * W) and np.all(sums[:, 3] == ((H - 10) * (W - 10) if H > 10 and W > 10 else 1))
        if v is not None:
            assert np.array_equal(v.view(np.int32), ref[kernel][1].view(np.int32)), kernel


# ---------------------------------------------------------------------------------------------------------------------
# 3. zero weight means zero influence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
@pytest.mark.parametrize("shape", [(1, 23, 70), (2, 141, 139), (1, 257, 75)], ids=_ids)
def test_zero_weight_means_zero_influence(ctx, shape, content):
    """Weights that are zero on a rectangle R (which crosses strip and band edges), uniform elsewhere.  A ground truth
    changed (finite values far outside [0, 1]) on R eroded by 5 px: no window of a pixel outside R reaches it."""
    Cn, H, W = shape
    x, y = images(shape, content)
    r0, r1, c0, c1 = H // 5, H // 5 + max(13, H // 2), W // 4, W // 4 + max(13, W // 2)
    assert r1 < H and c1 < W
    w = lmc.weights_for("uniform", Cn, H, W, 5).copy()
    w[:, r0:r1, c0:c1] = 0.0
    inner = np.zeros((H, W), bool); inner[r0 + 5:r1 - 5, c0 + 5:c1 - 5] = True
    assert inner.any()
    y2 = y.copy()
    y2[:, inner] = np.random.default_rng(1).uniform(-50.0, 50.0, y2[:, inner].shape).astype(np.float32)
    a = run_weighted(ctx, dev(x), dev(y), dev(w))
    b = run_weighted(ctx, dev(x), dev(y2), dev(w))
    for kernel in KERNELS:
        assert np.array_equal(a[kernel][0].view(np.int64), b[kernel][0].view(np.int64)), kernel
        if a[kernel][1] is not None:
            va, vb = a[kernel][1], b[kernel][1]
            assert np.array_equal(va[:, ~inner].view(np.int32), vb[:, ~inner].view(np.int32)), kernel
            assert np.all(va[:, inner] == 0) and np.all(vb[:, inner] == 0), kernel
            assert np.abs(va[:, ~inner]).max() > 0


@pytest.mark.parametrize("shape", [(1, 23, 70), (2, 141, 139)], ids=_ids)
def test_a_view_without_weight_gets_zero_sums_and_a_zero_gradient(ctx, shape):
    Cn, H, W = shape
    x, y = images(shape, "structured")
    w = lmc.weights_for("zero_view", Cn, H, W, 3)
    res = run_weighted(ctx, dev(x), dev(y), dev(w))
    for kernel in KERNELS:
        sums, v = res[kernel]
        assert np.all(sums[-1, :2] == 0.0) and np.all(sums[-1, 2:] == 1.0), (kernel, sums)
        if v is not None:
            assert np.all(v[-1] == 0.0), kernel
            assert Cn == 1 or np.abs(v[0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. fused equals unfused
# ---------------------------------------------------------------------------------------------------------------------
def _scene_weights(Cn, H, W, seed=11):
    """uniform in [0, 2] with a zero rectangle, every view its own draw"""
    w = lmc.weights_for("uniform", Cn, H, W, seed).copy()
    w[:, H // 4:H // 2, W // 3:2 * W // 3] = 0.0
    return dev(w)


def _loss_of_sums(sums, Wt, ssim_fac):
    """k_finalize_loss's formula on the per-view sums of the weighted loss, in double"""
    H, W = Wt.shape[1:]
    w_ssim = float(np.float32(ssim_fac)); w_l1 = float(np.float32(1.0) - np.float32(ssim_fac))
    s = sums.cpu().numpy()
    sum_i = Wt[:, 5:H - 5, 5:W - 5].double().sum((1, 2)).cpu().numpy()
    return sum(w_l1 * s[c, 0] / (3 * s[c, 2]) + w_ssim * (3 * sum_i[c] - s[c, 1]) / (3 * s[c, 3]) for c in range(s.shape[0]))


def _unfused(ctx, P, vm, K, gt, Wt, W, H, ssim_fac, E=None, prior=None):
    """rasterization -> (exposure) -> weighted loss -> (exposure backward, depth prior) -> blend backward -> projection
    backward: the stand-alone calls in the fused step's order -> grads [23N], v_exposure or None, the loss in double"""
    from starst3r_amd import ops
    Cn = vm.shape[0]
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    y = rgb if E is None else ops.exposure_fwd(ctx, rgb, E)
    sums, v_x = ops.loss_l1_ssim_weighted(ctx, y, gt, Wt, 1.0 - ssim_fac, ssim_fac)
    loss = _loss_of_sums(sums, Wt, ssim_fac)
    v_E = None
    if E is not None:
        v_x, v_E = ops.exposure_bwd(ctx, rgb, E, v_x)
    v_a = v_d = None
    if prior is not None:
        d = ops.blend_depth_fwd(ctx, *lists, alpha, info["_last_ids"], Cn, W, H)
        dsums, v_d, v_a = ops.loss_depth_prior(ctx, d, alpha, prior[0], prior[1], DEPTH_FAC)
        ds = dsums.cpu().numpy()
        loss += float(np.float32(DEPTH_FAC)) * float((ds[:, 0] / ds[:, 1]).sum())
    ops.blend_fwd(ctx, *lists, Cn, W, H)
    vs = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_x, v_a, info["_cum_tiles"], Cn, W, H)
    if prior is not None:
        vs.add_(ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], v_d, info["_cum_tiles"], Cn, W, H))
    grads = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, info["_campos"], W,
                               H, info["_splats"], vs)
    if prior is not None:
        ops.depth_bwd(ctx, P["means"], vm, info["_splats"], vs, grads, None)
    torch.cuda.synchronize()
    return grads, v_E, loss


def _fused(ctx, P, vm, K, campos, gt, Wt, W, H, ssim_fac, debug=0):
    from starst3r_amd import ops
    N = P["means"].shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    ops.set_loss_weight(ctx, gt, Wt)
    ops.set_debug(ctx, debug)
    try:
        ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, ssim_fac, 0.0, 0.0, grads, loss)
    finally:
        ops.set_debug(ctx, 0)
        ops.set_loss_weight(ctx, None, None)
    torch.cuda.synchronize()
    return grads, float(loss)


@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_step_equals_unfused_chain(name):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    Wt = _scene_weights(Cn, H, W)
    grads_u, _, loss_u = _unfused(ctx, P, vm, K, gt, Wt, W, H, 0.2)
    grads_f, loss_f = _fused(ctx, P, vm, K, campos, gt, Wt, W, H, 0.2)
    print(name, "fused vs unfused: grads max |d| %.1e, loss %.9g vs %.9g"
          % (float((grads_f - grads_u).abs().max()), loss_f, loss_u))
    assert float(grads_u.abs().max()) > 0 and _same_bits(grads_f, grads_u), name
    assert abs(loss_f - loss_u) <= 1e-6 * abs(loss_u), (name, loss_f, loss_u)
    # the weights do something: without the registration the gradient is another one, and a cleared one is that call
    grads_p = torch.empty_like(grads_u); loss_p = torch.zeros(1, device="cuda:0")
    ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads_p, loss_p)
    torch.cuda.synchronize()
    assert not _same_bits(grads_p, grads_f)
    if name == "many":   # 9 views in chunks of 4 and 5 (debug flag 32): the agreement of the exposure test
        grads_c, loss_c = _fused(ctx, P, vm, K, campos, gt, Wt, W, H, 0.2, debug=32)
        rel = float((grads_c - grads_f).abs().max() / grads_f.abs().max())
        print("many, two view chunks: grads max rel %.1e, loss %.9g vs %.9g" % (rel, loss_c, loss_f))
        assert rel < 1e-6
        assert loss_c == pytest.approx(loss_f, rel=1e-6)
    ctx.close()


def test_registration_combines_with_exposures_depth_prior_and_poses():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    Wt = _scene_weights(Cn, H, W)
    gen = torch.Generator().manual_seed(77)
    E = (torch.eye(3, 4).repeat(Cn, 1, 1) + 0.1 * torch.randn((Cn, 3, 4), generator=gen)).contiguous().cuda()
    prior = _synthetic_prior(ctx, P, vm, K, W, H)[:2]
    grads_u, vE_u, loss_u = _unfused(ctx, P, vm, K, gt, Wt, W, H, 0.2, E=E, prior=prior)
    r = _Run(P, vm, campos, 1)
    vE = torch.full_like(E, 7.0)
    ops.set_exposure(ctx, gt, E, vE)
    ops.set_depth_prior(ctx, gt, prior[0], prior[1], DEPTH_FAC)
    ops.set_loss_weight(ctx, gt, Wt)
    try:   # learning rates 0: gradients and loss only
        ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.0, 0.0, r.grads, r.m, r.v, 0.0, B1, B2, EPS, 1,
                             r.losses[0:1], r.pm, r.pv, 0.0, 1, None, r.vvm)
    finally:
        ops.set_exposure(ctx, None, None, None); ops.set_depth_prior(ctx, None, None, None)
        ops.set_loss_weight(ctx, None, None)
    torch.cuda.synchronize()
    print("combined: grads max |d| %.1e, v_exposure max |d| %.1e, loss %.9g vs %.9g"
          % (float((r.grads - grads_u).abs().max()), float((vE - vE_u).abs().max()), float(r.losses[0]), loss_u))
    assert _same_bits(r.grads, grads_u) and _same_bits(vE, vE_u)
    assert abs(float(r.losses[0]) - loss_u) <= 1e-6 * abs(loss_u)
    assert float(r.vvm.abs().max()) > 0 and float(vE_u.abs().min()) > 0
    ctx.close()


def test_the_bindings_check_their_tensors_and_keep_them_alive():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Wt = _scene_weights(vm.shape[0], H, W)
    ops.set_loss_weight(ctx, gt, Wt)
    assert ctx._lw_keep is not None
    with pytest.raises(AssertionError):   # a map of another size is refused by the binding
        ops.set_loss_weight(ctx, gt, Wt[:, :-1].contiguous())
    ops.set_loss_weight(ctx, None, None)
    assert ctx._lw_keep is None
    with pytest.raises(ValueError):
        ops.loss_l1_ssim_weighted(ctx, gt, gt, Wt.double(), 0.8, 0.2)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
def test_cleared_and_all_ones_registrations_change_nothing():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P0, vm, K, campos, gt, W, H = _medium(ctx)
    Cn, steps = vm.shape[0], 3

    def run(register):
        r = _Run(P0, vm, campos, steps)
        register()
        try:
            for it in range(steps):
                ops.train_step(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS,
                               it + 1, r.losses[it:it + 1])
        finally:
            ops.set_loss_weight(ctx, None, None)
        torch.cuda.synchronize()
        return r

    a = run(lambda: None)
    ones = torch.ones((Cn, H, W), device="cuda:0")

    def set_and_clear():
        ops.set_loss_weight(ctx, gt, ones)
        ops.set_loss_weight(ctx, None, None)

    c = run(set_and_clear)
    for k in a.P:
        assert _same_bits(a.P[k], c.P[k]), k
    assert _same_bits(a.m, c.m) and _same_bits(a.v, c.v) and _same_bits(a.losses, c.losses)
    b = run(lambda: ops.set_loss_weight(ctx, gt, ones))
    for k in a.P:
        assert _same_bits(a.P[k], b.P[k]), k
    assert _same_bits(a.m, b.m) and _same_bits(a.v, b.v)
    la, lb = a.losses.cpu().numpy(), b.losses.cpu().numpy()
    print("all-ones registration: losses", la, lb)
    assert np.all(np.abs(la - lb) <= np.spacing(np.abs(la)))
    # and real weights move them
    d = run(lambda: ops.set_loss_weight(ctx, gt, _scene_weights(Cn, H, W)))
    assert not _same_bits(a.P["means"], d.P["means"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. through run_3dgs_optim
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_noise_does_not_reach_the_gaussians_through_run_3dgs_optim(ctx):
    """"small": 3 views of 96 x 64, 400 Gaussians; the photographs are the scene's own render from perturbed Gaussians.
    loss_masks is zero on a 40 x 34 rectangle per view; the inner 30 x 24 of it (the rectangle eroded by the 5 px a window
    reaches) is replaced by noise in a second set of photographs."""
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("small")
    V, iters = w2c.shape[0], 10
    P = {k: dev(v) for k, v in g.items()}
    vm = dev(w2c)
    rgb, _, _ = ops.render(ctx, P, vm, dev(Ks), ops.camera_positions(vm), W, H)
    clean = rgb.cpu().numpy()
    g_start = synth.perturb_for_gt(g)
    r0, c0 = 12, 30                          # the rectangle: rows 12 .. 45, columns 30 .. 69
    masks = []
    for v in range(V):
        m = np.ones((H, W), np.float32)
        m[r0:r0 + 34, c0:c0 + 40] = 0.0
        masks.append(m)
    noisy = clean.copy()
    noisy[:, r0 + 5:r0 + 29, c0 + 5:c0 + 35] = np.random.default_rng(2).uniform(0, 1, (V, 24, 30, 3)).astype(np.float32)

    def run(imgs, use_masks, **kw):
        scene = _optim_scene(g_start, torch.tensor(w2c), Ks, imgs)
        if use_masks:
            scene.loss_masks = masks
        losses = scene.run_3dgs_optim(iters, enable_pruning=False, **kw)
        torch.cuda.synchronize()
        return scene, losses

    a, la = run(clean, True)
    b, lb = run(noisy, True)
    for k in a.gaussians:
        assert _same_bits(a.gaussians[k].data, b.gaussians[k].data), k
    assert not _same_bits(a.gaussians["means"].data, dev(g_start["means"]))   # (they trained)
    print("run_3dgs_optim with masks: losses", la[0], "->", la[-1], "| noisy", lb[0], "->", lb[-1])
    assert len(la) == iters and np.allclose(la, lb, rtol=1e-6, atol=0)
    assert ops.get_context("cuda:0")._lw_keep is None   # the registration belongs to the call
    # without masks the noise reaches the Gaussians
    c, lc = run(clean, False)
    d, ld = run(noisy, False)
    assert not _same_bits(c.gaussians["means"].data, d.gaussians["means"].data)
    assert not np.allclose(lc, ld, rtol=1e-6, atol=0)
    assert not _same_bits(a.gaussians["means"].data, c.gaussians["means"].data)   # (and the masks change the training)
    # all entries None: off -- the bits of a scene without the setting
    e = _optim_scene(g_start, torch.tensor(w2c), Ks, clean)
    e.loss_masks = [None] * V
    le = e.run_3dgs_optim(iters, enable_pruning=False)
    assert _same_bits(e.gaussians["means"].data, c.gaussians["means"].data) and le == lc
    assert getattr(e, "_loss_mask_dev", None) is None
    # together with the exposures and the poses
    c2w0 = torch.inverse(torch.as_tensor(w2c).double()).float()
    f, lf = run(noisy, True, exposure_lr=1e-3, exposure_freeze=(0,), pose_lr=1e-4, pose_freeze=(0,))
    assert len(lf) == iters and all(np.isfinite(lf))
    eye = torch.eye(3, 4, device="cuda:0")
    assert _same_bits(f.exposures[0], eye) and all(not _same_bits(f.exposures[v], eye) for v in range(1, V))
    assert _same_bits(f.c2w[0], c2w0[0]) and all(not torch.equal(f.c2w[v].cpu(), c2w0[v]) for v in range(1, V))
