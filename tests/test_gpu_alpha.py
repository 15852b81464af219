"""GPU tests of the backgrounds and the alpha supervision: the two streaming kernels of csrc/gs_alpha.hip through
st3r_composite_fwd / st3r_alpha_grad, render_3dgs under scene.render_backgrounds, the registrations st3r_ctx_set_background /
st3r_ctx_set_alpha_target in the fused training calls, and scene.backgrounds / scene.alpha_fac through run_3dgs_optim.

    1. the kernels against the reference of tests/alpha_cases.py, bit for bit      4. the fused step equals the unfused chain
    2. the forward on arbitrary floats                                             5. nothing else moves
    3. autograd through render_3dgs                                                6. through run_3dgs_optim
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import alpha_cases as ac
from per_view_cases import (B1, B2, EPS, _Run, _medium, _optim_scene, _same_bits, _setup, _synthetic_prior, dev, make,
                            rel_err_per_camera)
from per_view_kernel_cases import STREAM_SHAPES, shape_tags
from st3r_synth import synth

ALPHA_FAC = 0.5
DEPTH_FAC = 0.5


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def _ids(s):
    return "x".join(map(str, s))


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs and references of one shape; computed once, modified by nobody"""
    d = ac.inputs(shape)
    for a in d.values():
        a.setflags(write=False)
    refs = {}
    for bg in (False, True):
        for at in (False, True):
            for acc in (False, True):
                if bg or at:
                    refs[bg, at, acc] = ac.alpha_grad_reference(
                        d["alpha"], d["b"] if bg else None, d["v"] if bg else None, d["M"] if at else None,
                        d["w"] if at else None, ac.ALPHA_FAC, d["v_in"] if acc else None)
    return d, ac.composite_reference(d["x"], d["alpha"], d["b"]), refs


def _placed(a, how):
    """the array on the device: "plain", "view" (views 1 .. C of a [C + 1, ...] buffer) or "shifted" (one float into a buffer)"""
    t = dev(a)
    if how == "plain":
        return t
    if how == "view":
        buf = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), 7.0, device="cuda:0")
        buf[1:].copy_(t)
        return buf[1:]
    buf = torch.full((t.numel() + 1,), 7.0, device="cuda:0")
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the reference
# ---------------------------------------------------------------------------------------------------------------------
PLACEMENTS = [(s, "plain") for s in STREAM_SHAPES] + [((2, 33, 63), "view"), ((3, 33, 32), "shifted")]


@pytest.mark.parametrize("shape,how", PLACEMENTS, ids=lambda p: _ids(p) if isinstance(p, tuple) else p)
def test_kernels_give_the_bits_of_the_reference(ctx, shape, how):
    from starst3r_amd import ops
    C, H, W = shape
    d, y_ref, refs = case(shape)
    if how == "view":
        assert (H * W) % 4 != 0
    if how == "shifted":
        assert (H * W) % 4 == 0                                      # the vector form is refused by the pointers alone
    T = {k: _placed(d[k], "plain" if k == "b" else how) for k in ("x", "alpha", "b", "v", "M", "w", "v_in")}
    if how != "plain":
        assert T["alpha"].data_ptr() % 16 != 0 and T["alpha"].is_contiguous()
    print("ALPHA", _ids(shape), how, shape_tags(shape, how == "plain"))
    # the composite, into a buffer of its own and in place
    y = ops.composite_fwd(ctx, T["x"], T["alpha"], T["b"])
    x2 = _placed(d["x"], how)
    assert ops.composite_fwd(ctx, x2, T["alpha"], T["b"], out=x2) is x2
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(y.cpu().numpy()), _bits32(y_ref)) and _same_bits(x2, y)
    assert _same_bits(T["x"], dev(d["x"]))                           # the input of the out-of-place call is untouched
    # every switch combination of alpha_grad
    on = d["on"]
    for (bg, at, acc), ref in refs.items():
        kw = dict(backgrounds=T["b"] if bg else None, v_out=T["v"] if bg else None, target=T["M"] if at else None,
                  weight=T["w"] if at else None, alpha_fac=ac.ALPHA_FAC)
        tag = (_ids(shape), how, bg, at, acc)
        runs = [dict(v_alpha_in=T["v_in"] if acc else None)]
        if acc:                                                      # in place: v_alpha is v_alpha_in
            buf = _placed(d["v_in"], how)
            runs.append(dict(v_alpha_in=buf, v_alpha=buf))
        for extra in runs:
            v_alpha, sums, v_b = ops.alpha_grad(ctx, T["alpha"], want_v_backgrounds=True, **kw, **extra)
            torch.cuda.synchronize()
            if "v_alpha" in extra:
                assert v_alpha is extra["v_alpha"]
            va = v_alpha.cpu().numpy()
            assert np.array_equal(_bits32(va), _bits32(ref["v_alpha"])), tag
            assert (sums is not None) == at and (v_b is not None) == bg
            if at:
                s = sums.cpu().numpy()
                assert np.array_equal(s[:, 0].view(np.int64), ref["sums"].view(np.int64)), (tag, s[:, 0], ref["sums"])
                assert np.array_equal(s[:, 1].view(np.int64), ref["n_c"].view(np.int64)), (tag, s[:, 1], ref["n_c"])
                if not bg and not acc:                               # a pixel without weight: exact zeros, NaN in M or not
                    assert np.all(va[..., 0][~on] == 0) and not np.isfinite(d["M"][~on]).any()
            if bg:
                assert np.array_equal(_bits32(v_b.cpu().numpy()), _bits32(ref["v_b"])), (tag, v_b, ref["v_b"])
        if bg and not at and not acc:                                # without v_backgrounds: the same v_alpha, no sums formed
            v2, _, none = ops.alpha_grad(ctx, T["alpha"], **kw)
            assert none is None and np.array_equal(_bits32(v2.cpu().numpy()), _bits32(ref["v_alpha"]))
    assert _same_bits(T["v_in"], dev(d["v_in"])) and _same_bits(T["alpha"], dev(d["alpha"]))


def test_the_bindings_check_their_tensors_and_keep_them_alive():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    d, _, _ = case((3, 33, 32))
    T = {k: dev(d[k]) for k in ("x", "alpha", "b", "v", "M", "w")}
    with pytest.raises(ValueError):                                  # no term at all: refused by the binding ...
        ops.alpha_grad(ctx, T["alpha"])
    from starst3r_amd import _lib
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.empty_like(T["alpha"])
    rc = _lib.lib().st3r_alpha_grad(ctx.handle, None, 3, 33, 32, p(T["alpha"]), None, None, None, None, 1.0, None, None, p(out),
                                    None)
    assert rc == -1                                                  # ... and by the library: ST3R_ERR_INVALID
    with pytest.raises(ValueError):
        ops.alpha_grad(ctx, T["alpha"], backgrounds=T["b"])         # half a term
    with pytest.raises(ValueError):
        ops.alpha_grad(ctx, T["alpha"], target=T["M"], weight=T["w"].double(), alpha_fac=1.0)
    with pytest.raises(ValueError):
        ops.composite_fwd(ctx, T["x"], T["alpha"], T["b"][:2].contiguous())
    with pytest.raises(ValueError):
        ops.alpha_grad(ctx, T["alpha"], target=T["M"], weight=T["w"], alpha_fac=float("nan"))
    gt = T["x"]
    ops.set_background(ctx, gt, T["b"]); ops.set_alpha_target(ctx, gt, T["M"], T["w"], 1.0)
    assert ctx._bg_keep is not None and ctx._at_keep is not None
    with pytest.raises(AssertionError):
        ops.set_background(ctx, gt, T["b"][:2].contiguous())
    with pytest.raises(AssertionError):
        ops.set_alpha_target(ctx, gt, T["M"][:, :-1].contiguous(), T["w"], 1.0)
    with pytest.raises(ValueError):
        ops.set_alpha_target(ctx, gt, T["M"], T["w"], float("inf"))
    ops.set_background(ctx, None, None); ops.set_alpha_target(ctx, None, None, None)
    assert ctx._bg_keep is None and ctx._at_keep is None
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the forward on arbitrary floats
# ---------------------------------------------------------------------------------------------------------------------
def test_composite_of_a_real_render_against_float64(ctx):
    """y = fmaf(1 - a, b, x): one rounding of 1 - a (relative 2^-24, times |b| <= its absolute share) and one of the fma
    (half a unit of the result)"""
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("ragged")
    P = {k: dev(v) for k, v in g.items()}
    vm = dev(w2c)
    rgb, alpha, _ = ops.render(ctx, P, vm, dev(Ks), ops.camera_positions(vm), W, H)
    b = torch.tensor([[1.0, 1.0, 1.0], [0.3, 0.7, 0.123]], device="cuda:0")
    y = ops.composite_fwd(ctx, rgb, alpha, b).cpu().numpy().astype(np.float64)
    x64, a64, b64 = rgb.double().cpu().numpy(), alpha.double().cpu().numpy(), b.double().cpu().numpy()
    ref = x64 + (1.0 - a64) * b64[:, None, None, :]
    bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) / 2 + np.abs(b64)[:, None, None, :] * 2.0 ** -24
    err = np.abs(y - ref)
    print("composite of ragged: max err %.2e, max err / bound %.3f" % (err.max(), (err / bound).max()))
    assert float(alpha.min()) < 0.5 and float(alpha.max()) > 0.9     # (the background shows and is covered)
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------------------------
# 3. autograd
# ---------------------------------------------------------------------------------------------------------------------
def _render_scene(name):
    g, w2c, Ks, W, H = make(name)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, np.zeros((w2c.shape[0], H, W, 3), np.float32))
    return scene, torch.tensor(w2c), torch.tensor(Ks), W, H


def _dyadic(shape, unit, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return dev((rng.integers(lo * unit, hi * unit + 1, shape) / float(unit)).astype(np.float32))


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_render_3dgs_backgrounds_back_propagate_like_the_composition_by_hand(name):
    scene, w2c, Ks, W, H = _render_scene(name)
    V = w2c.shape[0]
    b0 = _dyadic((V, 3), 16, 0, 1, 5)
    v = _dyadic((V, H, W, 3), 8, -2, 2, 6)

    def grads(by_hand):
        for p in scene.gaussians.values():
            p.grad = None
        w = w2c.clone().cuda().requires_grad_()
        b = b0.clone().requires_grad_()
        scene.render_backgrounds = None if by_hand else b
        if by_hand:
            rgb, alpha, _ = scene.render_3dgs(w, Ks, W, H)
            img = rgb + (1 - alpha) * b[:, None, None, :]
        else:
            img, alpha, _ = scene.render_3dgs(w, Ks, W, H)
        (img * v).sum().backward()
        torch.cuda.synchronize()
        out = {k: p.grad.clone() for k, p in scene.gaussians.items() if p.grad is not None}
        return img.detach(), alpha.detach(), out, w.grad.clone(), b.grad.clone()

    img_h, alpha, g_h, w_h, b_h = grads(True)
    img_k, alpha_k, g_k, w_k, b_k = grads(False)
    assert _same_bits(alpha, alpha_k)
    assert sorted(g_h) == sorted(g_k) and float(g_h["means"].abs().max()) > 0 and float(w_h.abs().max()) > 0
    for k in g_h:
        assert _same_bits(g_h[k], g_k[k]), (name, k, float((g_h[k] - g_k[k]).abs().max()))
    assert _same_bits(w_h, w_k), (name, float((w_h - w_k).abs().max()))
    # the image: one fma against torch's multiply and add
    assert float((img_h - img_k).abs().max()) <= 2.0 ** -22
    # d loss / d backgrounds: the double sum of the float32 products (1 - a) v, stored as float32
    ref = ((1.0 - alpha).double() * v.double()).sum((1, 2))
    rel = float(((b_k.double() - ref).abs() / ref.abs().clamp(min=1e-30)).max())
    print(name, "b.grad", b_k.tolist(), "rel err %.2e (by hand %.2e)" % (rel, float(((b_h.double() - ref).abs() / ref.abs()).max())))
    assert rel <= 1e-6


def test_render_modes_with_backgrounds_and_exposure(ctx):
    from starst3r_amd import ops
    scene, w2c, Ks, W, H = _render_scene("small")
    V = w2c.shape[0]
    b = _dyadic((V, 3), 16, 0, 1, 5)
    gen = torch.Generator().manual_seed(3)
    E = (torch.eye(3, 4).repeat(V, 1, 1) + 0.1 * torch.randn((V, 3, 4), generator=gen)).cuda()
    with torch.no_grad():
        plain, alpha0, _ = scene.render_3dgs(w2c, Ks, W, H, render_mode="RGB+ED")
        depth_d, _, _ = scene.render_3dgs(w2c, Ks, W, H, "RGB+D")                     # render_mode keeps its positional slot
        scene.render_backgrounds = b
        both, alpha1, _ = scene.render_3dgs(w2c, Ks, W, H, render_mode="RGB+ED", exposure=E)
        only_b, _, _ = scene.render_3dgs(w2c, Ks, W, H, "RGB+D")
    assert tuple(both.shape) == (V, H, W, 4) and _same_bits(alpha0, alpha1)
    assert _same_bits(both[..., 3], plain[..., 3]) and _same_bits(only_b[..., 3], depth_d[..., 3])   # no background under the depth
    comp = ops.composite_fwd(ctx, plain[..., :3].contiguous(), alpha0, b)
    assert _same_bits(only_b[..., :3], comp)
    assert _same_bits(both[..., :3], ops.exposure_fwd(ctx, comp, E))                                 # scene first, then camera
    assert not _same_bits(comp, plain[..., :3])
    for mode in ("D", "ED"):
        with pytest.raises(ValueError, match="render_mode"):
            scene.render_3dgs(w2c, Ks, W, H, render_mode=mode)
    # and a gradient flows through all of it, the intrinsics included when asked for
    scene.intrinsics_grad = True
    K = Ks.clone().cuda().requires_grad_()
    bb = b.clone().requires_grad_()
    scene.render_backgrounds = bb
    img, _, _ = scene.render_3dgs(w2c, K, W, H, render_mode="RGB+ED", exposure=E)
    img.sum().backward()
    assert float(K.grad.abs().max()) > 0 and float(bb.grad.abs().min()) > 0 and float(scene.gaussians["means"].grad.abs().max()) > 0
    scene.backgrounds = b.cpu().numpy()
    with torch.no_grad():
        scene.render_backgrounds = True                                               # stands for scene.backgrounds
        orig, _, _ = scene.render_3dgs_original(W, H)
        scene.render_backgrounds = b
        direct, _, _ = scene.render_3dgs(scene.w2c, scene.intrinsics, W, H)
        scene.render_backgrounds = None
        off, _, _ = scene.render_3dgs_original(W, H)
    assert _same_bits(orig, direct) and not _same_bits(orig, off)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fused equals unfused
# ---------------------------------------------------------------------------------------------------------------------
def _scene_backgrounds(Cn, seed=8):
    gen = torch.Generator().manual_seed(seed)
    b = torch.rand((Cn, 3), generator=gen)
    b[0] = 1.0                                                       # white, and arbitrary colours
    return b.cuda().contiguous()


def _scene_targets(ctx, P, vm, K, W, H, seed=9):
    """targets: the render's own alpha, thresholded at 0.5 on the left half and perturbed on the right; weights uniform in
    [0, 2] with a zero rectangle, the last view without a target weight on its upper half"""
    from starst3r_amd import ops
    _, alpha, _ = ops.render(ctx, P, vm, K, ops.camera_positions(vm), W, H)
    a = alpha[..., 0]
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    M = torch.clamp(a + 0.2 * torch.randn(a.shape, device="cuda:0", generator=gen), 0, 1)
    M[:, :, :W // 2] = (a[:, :, :W // 2] > 0.5).float()
    w = 2.0 * torch.rand(a.shape, device="cuda:0", generator=gen)
    w[:, H // 4:H // 2, W // 3:2 * W // 3] = 0.0
    w[-1, :H // 2] = 0.0
    return M.contiguous(), w.contiguous()


def _plain_loss_of_sums(sums, H, W, ssim_fac):
    """k_finalize_loss's formula on the per-view sums of the unweighted loss, in double"""
    w_ssim = float(np.float32(ssim_fac)); w_l1 = float(np.float32(1.0) - np.float32(ssim_fac))
    s = sums.cpu().numpy()
    inv_px, inv_cnt = 1.0 / (H * W * 3.0), 1.0 / ((H - 10) * (W - 10) * 3.0)
    return sum(w_l1 * s[c, 0] * inv_px + w_ssim * (1.0 - s[c, 1] * inv_cnt) for c in range(s.shape[0]))


def _weighted_loss_of_sums(sums, Wt, ssim_fac):
    H, W = Wt.shape[1:]
    w_ssim = float(np.float32(ssim_fac)); w_l1 = float(np.float32(1.0) - np.float32(ssim_fac))
    s = sums.cpu().numpy()
    sum_i = Wt[:, 5:H - 5, 5:W - 5].double().sum((1, 2)).cpu().numpy()
    return sum(w_l1 * s[c, 0] / (3 * s[c, 2]) + w_ssim * (3 * sum_i[c] - s[c, 1]) / (3 * s[c, 3]) for c in range(s.shape[0]))


def _unfused(ctx, P, vm, K, gt, W, H, ssim_fac, b=None, at=None, E=None, prior=None, Wt=None, pose=False):
    """The stand-alone calls in the fused step's order: rasterization -> composite -> exposure -> loss -> exposure backward
    -> depth prior -> alpha_grad -> blend backward (-> depth blend backward) -> projection backward
    -> grads [23N], v_exposure or None, the loss in double (and with pose=True, no prior: v_viewmats of ops.viewmat_bwd)"""
    from starst3r_amd import ops
    Cn = vm.shape[0]
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    x = rgb if b is None else ops.composite_fwd(ctx, rgb, alpha, b)
    y = x if E is None else ops.exposure_fwd(ctx, x, E)
    if Wt is None:
        sums, v_x = ops.loss_l1_ssim(ctx, y, gt, 1.0 - ssim_fac, ssim_fac)
        loss = _plain_loss_of_sums(sums, H, W, ssim_fac)
    else:
        sums, v_x = ops.loss_l1_ssim_weighted(ctx, y, gt, Wt, 1.0 - ssim_fac, ssim_fac)
        loss = _weighted_loss_of_sums(sums, Wt, ssim_fac)
    v_E = None
    if E is not None:
        v_x, v_E = ops.exposure_bwd(ctx, x, E, v_x)
    v_a = v_d = None
    if prior is not None:
        d = ops.blend_depth_fwd(ctx, *lists, alpha, info["_last_ids"], Cn, W, H)
        dsums, v_d, v_a = ops.loss_depth_prior(ctx, d, alpha, prior[0], prior[1], DEPTH_FAC)
        ds = dsums.cpu().numpy()
        loss += float(np.float32(DEPTH_FAC)) * float((ds[:, 0] / ds[:, 1]).sum())
    if b is not None or at is not None:
        v_a, asums, _ = ops.alpha_grad(ctx, alpha, b, v_x if b is not None else None, None if at is None else at[0],
                                       None if at is None else at[1], ALPHA_FAC, v_alpha_in=v_a)
        if at is not None:
            s = asums.cpu().numpy()
            loss += float(np.float32(ALPHA_FAC)) * float((s[:, 0] / s[:, 1]).sum())
    ops.blend_fwd(ctx, *lists, Cn, W, H)
    vs = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_x, v_a, info["_cum_tiles"], Cn, W, H)
    if prior is not None:
        vs.add_(ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], v_d, info["_cum_tiles"], Cn, W, H))
    grads = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, info["_campos"], W,
                               H, info["_splats"], vs)
    if prior is not None:
        ops.depth_bwd(ctx, P["means"], vm, info["_splats"], vs, grads, None)
    if pose:
        vvm = ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K, info["_campos"], W, H, info["_splats"], vs)
        torch.cuda.synchronize()
        return grads, v_E, loss, vvm
    torch.cuda.synchronize()
    return grads, v_E, loss


def _register(ctx, gt, b, at):
    from starst3r_amd import ops
    if b is not None:
        ops.set_background(ctx, gt, b)
    if at is not None:
        ops.set_alpha_target(ctx, gt, at[0], at[1], ALPHA_FAC)


def _clear(ctx):
    from starst3r_amd import ops
    ops.set_background(ctx, None, None); ops.set_alpha_target(ctx, None, None, None)


def _fused(ctx, P, vm, K, campos, gt, W, H, ssim_fac, b, at, debug=0):
    from starst3r_amd import ops
    N = P["means"].shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
    _register(ctx, gt, b, at)
    ops.set_debug(ctx, debug)
    try:
        ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, ssim_fac, 0.0, 0.0, grads, loss)
    finally:
        ops.set_debug(ctx, 0)
        _clear(ctx)
    torch.cuda.synchronize()
    return grads, float(loss)


@pytest.mark.parametrize("which", ["backgrounds", "alpha", "both"])
@pytest.mark.parametrize("name", ["small", "ragged", "many", "wide"])
def test_fused_step_equals_unfused_chain(name, which):
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    b = _scene_backgrounds(Cn) if which != "alpha" else None
    at = _scene_targets(ctx, P, vm, K, W, H) if which != "backgrounds" else None
    grads_u, _, loss_u = _unfused(ctx, P, vm, K, gt, W, H, 0.2, b=b, at=at)
    grads_f, loss_f = _fused(ctx, P, vm, K, campos, gt, W, H, 0.2, b, at)
    print(name, which, "fused vs unfused: grads max |d| %.1e, loss %.9g vs %.9g"
          % (float((grads_f - grads_u).abs().max()), loss_f, loss_u))
    assert float(grads_u.abs().max()) > 0 and _same_bits(grads_f, grads_u), (name, which)
    assert abs(loss_f - loss_u) <= 1e-6 * abs(loss_u), (name, which, loss_f, loss_u)
    # the raw render stays where st3r_ctx_peek finds it
    if b is not None:
        rgb, _, _ = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
        _fused(ctx, P, vm, K, campos, gt, W, H, 0.2, b, at)
        assert _same_bits(ops.peek(ctx, 8, rgb.numel(), torch.float32), rgb.reshape(-1))
    # the registration does something: without it the gradient is another one
    grads_p = torch.empty_like(grads_u); loss_p = torch.zeros(1, device="cuda:0")
    ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.0, 0.0, grads_p, loss_p)
    torch.cuda.synchronize()
    assert not _same_bits(grads_p, grads_f)
    if name == "many":   # 9 views in chunks of 4 and 5 (debug flag 32): the agreement of the exposure and mask tests
        grads_c, loss_c = _fused(ctx, P, vm, K, campos, gt, W, H, 0.2, b, at, debug=32)
        rel = float((grads_c - grads_f).abs().max() / grads_f.abs().max())
        print("many, two view chunks: grads max rel %.1e, loss %.9g vs %.9g" % (rel, loss_c, loss_f))
        assert rel < 1e-6
        assert loss_c == pytest.approx(loss_f, rel=1e-6)
    ctx.close()


def test_all_six_registrations_combine_and_v_alpha_accumulates_onto_the_depth_priors():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    Cn = vm.shape[0]
    import loss_mask_cases as lmc
    Wt = dev(lmc.weights_for("uniform", Cn, H, W, 11))
    gen = torch.Generator().manual_seed(77)
    E = (torch.eye(3, 4).repeat(Cn, 1, 1) + 0.1 * torch.randn((Cn, 3, 4), generator=gen)).contiguous().cuda()
    prior = _synthetic_prior(ctx, P, vm, K, W, H)[:2]
    b, at = _scene_backgrounds(Cn), _scene_targets(ctx, P, vm, K, W, H)
    grads_u, vE_u, loss_u = _unfused(ctx, P, vm, K, gt, W, H, 0.2, b=b, at=at, E=E, prior=prior, Wt=Wt)
    grads_n, _, _ = _unfused(ctx, P, vm, K, gt, W, H, 0.2, b=b, at=None, E=E, prior=prior, Wt=Wt)
    r = _Run(P, vm, campos, 1)
    vE = torch.full_like(E, 7.0); vK = torch.full((Cn, 4), 7.0, device="cuda:0")
    ops.set_exposure(ctx, gt, E, vE)
    ops.set_depth_prior(ctx, gt, prior[0], prior[1], DEPTH_FAC)
    ops.set_loss_weight(ctx, gt, Wt)
    ops.set_intrinsics_grad(ctx, gt, vK)
    _register(ctx, gt, b, at)
    try:   # learning rates 0: gradients and loss only
        ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.0, 0.0, r.grads, r.m, r.v, 0.0, B1, B2, EPS, 1,
                             r.losses[0:1], r.pm, r.pv, 0.0, 1, None, r.vvm)
    finally:
        ops.set_exposure(ctx, None, None, None); ops.set_depth_prior(ctx, None, None, None)
        ops.set_loss_weight(ctx, None, None); ops.set_intrinsics_grad(ctx, None, None)
        _clear(ctx)
    torch.cuda.synchronize()
    print("combined: grads max |d| %.1e, v_exposure max |d| %.1e, loss %.9g vs %.9g"
          % (float((r.grads - grads_u).abs().max()), float((vE - vE_u).abs().max()), float(r.losses[0]), loss_u))
    assert _same_bits(r.grads, grads_u) and _same_bits(vE, vE_u)
    assert not _same_bits(grads_n, grads_u)                          # (the alpha term is in there)
    assert abs(float(r.losses[0]) - loss_u) <= 1e-6 * abs(loss_u)
    assert float(r.vvm.abs().max()) > 0 and float(vE_u.abs().min()) > 0 and not bool((vK == 7.0).any())
    ctx.close()


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_poses_without_a_depth_prior_take_the_alpha_path_from_the_colour_slots(name):
    """train_step_poses with backgrounds and alpha targets and NO depth prior: need_pairs stays false, so the projection and
    the pose backward read the colour backward's slots, which here carry d loss / d alpha as well.  Rates 0: gradients only.
    The Gaussians' gradients are the unfused chain's bits (the same kernels on the same slots); the pose gradient is held to
    the bar of test_gpu_pose_train.py::test_fused_pose_gradient_equals_unfused_chain, 5e-5 of a camera's largest entry."""
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make(name)
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    b, at = _scene_backgrounds(vm.shape[0]), _scene_targets(ctx, P, vm, K, W, H)
    grads_u, _, loss_u, vvm_u = _unfused(ctx, P, vm, K, gt, W, H, 0.2, b=b, at=at, pose=True)
    _, _, _, vvm_plain = _unfused(ctx, P, vm, K, gt, W, H, 0.2, pose=True)
    r = _Run(P, vm, campos, 1)
    _register(ctx, gt, b, at)
    try:
        ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.0, 0.0, r.grads, r.m, r.v, 0.0, B1, B2, EPS, 1,
                             r.losses[0:1], r.pm, r.pv, 0.0, 1, None, r.vvm)
    finally:
        _clear(ctx)
    torch.cuda.synchronize()
    err = rel_err_per_camera(r.vvm, vvm_u)
    print(name, "poses, no prior: grads max |d| %.1e, pose gradient max |d| / max |ref| per camera %s, loss %.9g vs %.9g"
          % (float((r.grads - grads_u).abs().max()), ["%.1e" % e for e in err], float(r.losses[0]), loss_u))
    assert float(vvm_u.abs().max()) > 0 and max(rel_err_per_camera(vvm_plain, vvm_u)) > 1e-3    # the options move the poses' gradient
    assert _same_bits(r.grads, grads_u)
    assert max(err) <= 5e-5, (name, err)
    assert abs(float(r.losses[0]) - loss_u) <= 1e-6 * abs(loss_u)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
def test_cleared_registrations_change_nothing_and_real_ones_do():
    from starst3r_amd import ops
    ctx = ops.Context("cuda:0")
    P0, vm, K, campos, gt, W, H = _medium(ctx)
    Cn, steps = vm.shape[0], 3
    b, at = _scene_backgrounds(Cn), _scene_targets(ctx, P0, vm, K, W, H)

    def run(register):
        r = _Run(P0, vm, campos, steps)
        register()
        try:
            for it in range(steps):
                ops.train_step(ctx, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS,
                               it + 1, r.losses[it:it + 1])
        finally:
            _clear(ctx)
        torch.cuda.synchronize()
        return r

    def same(x, y):
        return all(_same_bits(x.P[k], y.P[k]) for k in x.P) and _same_bits(x.m, y.m) and _same_bits(x.v, y.v) and \
            _same_bits(x.losses, y.losses)

    a = run(lambda: None)

    def set_and_clear():
        _register(ctx, gt, b, at)
        _clear(ctx)

    assert same(a, run(set_and_clear))
    # alpha_fac = 0 is no registration either
    assert same(a, run(lambda: ops.set_alpha_target(ctx, gt, at[0], at[1], 0.0)))
    for reg in ((b, None), (None, at), (b, at)):
        d = run(lambda: _register(ctx, gt, *reg))
        assert not _same_bits(a.P["means"], d.P["means"]) and not _same_bits(a.losses, d.losses)
    assert same(a, run(lambda: None))                                # and the context is as it was
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. through run_3dgs_optim
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_object_training_through_run_3dgs_optim(ctx, monkeypatch):
    """"small": 3 views of 96 x 64, 400 Gaussians.  The photographs: the scene's own render over white, the left half of
    every view replaced by white -- an object segmented away.  loss_masks drops that half from the photometric loss;
    alpha_masks asks for alpha 0 there and for the render's own alpha on the right."""
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("small")
    V, iters = w2c.shape[0], 30
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, alpha, _ = ops.render(ctx, P, vm, K, campos, W, H)
    white = torch.ones((V, 3), device="cuda:0")
    photos = ops.composite_fwd(ctx, rgb, alpha, white).clamp(0, 1).cpu().numpy()
    photos[:, :, :W // 2] = 1.0
    own_alpha = alpha[..., 0].clamp(0, 1).cpu().numpy()
    loss_masks, alpha_masks = [], []
    for v in range(V):
        m = np.ones((H, W), np.float32); m[:, :W // 2] = 0.0
        t = own_alpha[v].copy(); t[:, :W // 2] = 0.0
        loss_masks.append(m); alpha_masks.append(t)
    g_start = synth.perturb_for_gt(g)

    def left_alpha(G):
        Pg = {k: (G[k].detach() if torch.is_tensor(G[k]) else dev(G[k])).contiguous()
              for k in ("means", "quats", "scales", "opacities", "shN")}
        _, a, _ = ops.render(ctx, Pg, vm, K, campos, W, H)
        return float(a[:, 5:H - 5, 5:W // 2 - 5].double().mean())   # the left half eroded by 5 px, the reach of an SSIM window

    def run(n_iters=iters, settings=True, **attrs):
        scene = _optim_scene(g_start, torch.tensor(w2c), Ks, photos)
        if settings:
            scene.loss_masks, scene.backgrounds = loss_masks, np.ones((V, 3), np.float32)
        for k, val in attrs.pop("scene_attrs", {}).items():
            setattr(scene, k, val)
        losses = scene.run_3dgs_optim(n_iters, loss_opacity_fac=0.0, loss_scale_fac=0.0, **attrs)
        torch.cuda.synchronize()
        return scene, losses

    start = left_alpha(g_start)
    on, l_on = run(scene_attrs=dict(alpha_fac=1.0, alpha_masks=alpha_masks))
    off, l_off = run(scene_attrs=dict(alpha_fac=0.0, alpha_masks=alpha_masks))
    a_on, a_off = left_alpha(on.gaussians), left_alpha(off.gaussians)
    print("mean alpha over the dropped half: start %.6f, alpha_fac = 1: %.6f, alpha_fac = 0: %.6f" % (start, a_on, a_off))
    print("losses: alpha_fac = 1: %.6f -> %.6f, alpha_fac = 0: %.6f -> %.6f" % (l_on[0], l_on[-1], l_off[0], l_off[-1]))
    assert len(l_on) == iters and all(np.isfinite(l_on))
    assert a_on < start and a_on < a_off
    assert l_on[0] > l_off[0]                                        # the returned losses include the alpha term
    c = ops.get_context("cuda:0")
    assert c._bg_keep is None and c._at_keep is None and c._lw_keep is None   # the registrations belong to the call
    # alpha_fac = 0 with masks set: the bits of a scene without the alpha settings
    none, l_none = run()
    for k in off.gaussians:
        assert _same_bits(off.gaussians[k].data, none.gaussians[k].data), k
    assert l_off == l_none and getattr(off, "_alpha_maps_dev", None) is None
    # with weights: "don't know" pixels
    weights = [np.ones((H, W), np.float32) for _ in range(V)]
    for wt in weights:
        wt[:, W // 2 - 8:W // 2 + 8] = 0.0
    tri, l_tri = run(scene_attrs=dict(alpha_fac=1.0, alpha_masks=alpha_masks, alpha_weights=weights))
    assert all(np.isfinite(l_tri)) and not _same_bits(tri.gaussians["means"].data, on.gaussians["means"].data)
    # scene.backgrounds all zero: the losses of the plain run (the parameters' bits are printed, not asserted: this step
    # takes k_blend_bwd<true> with an all-zero v_alpha, another kernel variant than the plain step)
    plain, l_plain = run(10, settings=False)
    zero, l_zero = run(10, settings=False, scene_attrs=dict(backgrounds=np.zeros((V, 3), np.float32)))
    same = {k: _same_bits(plain.gaussians[k].data, zero.gaussians[k].data) for k in plain.gaussians}
    print("zero backgrounds against the plain run: same parameter bits", same, "max |d means| %.2e"
          % float((plain.gaussians["means"].data - zero.gaussians["means"].data).abs().max()))
    assert np.allclose(l_zero, l_plain, rtol=1e-6, atol=0)
    # under enable_pruning, and together with the other options
    pr, l_pr = run(10, enable_pruning=True, scene_attrs=dict(alpha_fac=1.0, alpha_masks=alpha_masks))
    assert len(l_pr) == 10 and all(np.isfinite(l_pr))
    mix, l_mix = run(10, exposure_lr=1e-3, exposure_freeze=(0,), pose_lr=1e-4, pose_freeze=(0,), depth_fac=0.1,
                     scene_attrs=dict(alpha_fac=1.0, alpha_masks=alpha_masks, intrinsics_lr=1e-4, intrinsics_freeze=(0,),
                                      depth_maps=[torch.full((H, W), 3.0) for _ in range(V)]))
    assert len(l_mix) == 10 and all(np.isfinite(l_mix))
    # the sharded layout is refused
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError, match="backgrounds"):
        run(1, settings=False, scene_attrs=dict(backgrounds=np.ones((V, 3), np.float32)))
    with pytest.raises(NotImplementedError, match="alpha_fac"):
        run(1, settings=False, scene_attrs=dict(alpha_fac=1.0, alpha_masks=alpha_masks))


def test_the_example_of_masked_object_training():
    """examples/masked_object_training.py in small (3 views of 128 x 96, 100 iterations): the alpha term leaves less opacity
    outside the object than the same run without it -- a comparison between two runs from one seeding, no fixed number"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(__file__)), "examples", "masked_object_training.py")
    spec = importlib.util.spec_from_file_location("masked_object_training", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    without, with_alpha = mod.main(views=3, iters=100, W=128, H=96)
    print("mean alpha outside the object: alpha_fac 0 -> %.4f, alpha_fac 1 -> %.4f" % (without, with_alpha))
    assert np.isfinite(without) and np.isfinite(with_alpha) and with_alpha < without
