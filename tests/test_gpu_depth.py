"""Depth maps from render_3dgs (gsplat's render_mode "D" / "ED" / "RGB+D" / "RGB+ED") and their gradients:
st3r_gs_blend_depth_fwd / st3r_gs_blend_depth_bwd / st3r_gs_depth_bwd (gs_blend_depth.hip).

References: the CPU oracle's blend with per-pair colours (z, 0, 0) for the kernels, the existing colour kernels fed the same
depth-as-colour records, and float64 autograd through a dense depth render (below, on oracle/gs_torch_ref.project with
render_dense's weights) end to end.  Run on the MI355X box:
    python -m pytest tests/test_gpu_depth.py -m gpu -q
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as go
from oracle import gs_torch_ref as tr
from st3r_synth import synth
from test_gpu_gs import FUZZ_CHECKED
from per_view_cases import _gen, _pose_errors, _se3_exp, dev, make, rel_err_per_camera, run_hip

NAMED = ["small", "ragged", "medium", "one", "many", "wide"]
FUZZ3 = ["fuzz0", "fuzz1", "fuzz2"]


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def oracle_depth(g, w2c, Ks, W, H):
    """oracle colour render (for alpha, last_ids, margin) and its blend with per-pair colours (z, 0, 0)"""
    rgb_o, alpha_o, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"], w2c, Ks, W, H,
                                            want_margin=True)
    zcol = np.zeros((meta["depths"].shape[0], 3), np.float32)
    zcol[:, 0] = meta["depths"]
    d3, alpha_d, last_d, _ = go.blend_fwd(w2c.shape[0], W, H, 16, meta["means2d"], meta["conics"], zcol, meta["opacities"],
                                          meta["isect_offsets"], meta["flatten_ids"])
    assert np.array_equal(alpha_d, alpha_o) and np.array_equal(last_d, meta["last_ids"])
    return d3[..., 0:1], alpha_o, meta, zcol


def hip_depth(ctx, info, alpha, Cn, W, H):
    from starst3r_amd import ops
    d = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                            info["_last_ids"], Cn, W, H)
    torch.cuda.synchronize()
    return d


def depth_as_colour(info):
    """what a user could do before: a record copy whose colour is (z, 0, 0)"""
    s = info["_splats"].clone()
    s[:, 6] = s[:, 9]; s[:, 7] = 0.0; s[:, 8] = 0.0
    return s


# ---- 1. forward vs oracle ----
@pytest.mark.parametrize("name", NAMED + FUZZ3)
def test_depth_forward_vs_oracle(ctx, name):
    g, w2c, Ks, W, H = make(name)
    d_o, alpha_o, meta, _ = oracle_depth(g, w2c, Ks, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    d = hip_depth(ctx, info, alpha, w2c.shape[0], W, H).cpu().numpy()
    ok = meta["margin"] > 1e-4
    floor = FUZZ_CHECKED[name] - 2e-3 if name.startswith("fuzz") else 0.99
    print(name, "checked share %.4f, max z %.3f" % (ok.mean(), meta["depths"].max()))
    assert ok.mean() >= floor, (name, ok.mean())
    np.testing.assert_allclose(d[ok], d_o[ok], rtol=1e-4, atol=1e-5 * float(meta["depths"].max()))
    assert d_o.max() > 0


# ---- 2. forward vs the existing kernels: same decisions, so only the summation could differ ----
@pytest.mark.parametrize("name", NAMED + FUZZ3)
def test_depth_forward_vs_colour_kernel(ctx, name):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    Cn = w2c.shape[0]
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    d = hip_depth(ctx, info, alpha, Cn, W, H)
    rgb_z, alpha_z, last_z = ops.blend_fwd(ctx, depth_as_colour(info), info["isect_offsets"], info["_flatten_ids_dense"],
                                           Cn, W, H)
    torch.cuda.synchronize()
    assert torch.equal(alpha_z, alpha) and torch.equal(last_z, info["_last_ids"])
    ref = rgb_z[..., 0:1]
    err = float(((d - ref).abs() / ref.abs().clamp(min=1e-30)).max())
    print(name, "max relative difference to blend_fwd on (z, 0, 0):", err)
    np.testing.assert_allclose(d.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=0)   # measured: identical bits


# ---- 3. modes ----
def _scene(g):
    import starst3r_amd as st
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g.items()}
    return scene


def test_render_modes(ctx, monkeypatch):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("small")
    # camera 2 looks away from every Gaussian: nothing reaches its pixels
    w2c = w2c.copy()
    w2c[2] = synth.look_at_w2c((3.5, 0.0, 0.8), target=(10.0, 0.0, 0.8)).astype(np.float32)
    scene = _scene(g)
    w, K = dev(w2c), dev(Ks)
    with torch.no_grad():
        out = {m: scene.render_3dgs(w, K, W, H, render_mode=m) for m in ("RGB", "D", "ED", "RGB+D", "RGB+ED")}
        rgb, alpha, info = out["RGB"]
        assert rgb.shape == (3, H, W, 3) and alpha.shape == (3, H, W, 1)
        for m in ("RGB+D", "RGB+ED"):
            img, a, inf = out[m]
            assert img.shape == (3, H, W, 4) and inf.keys() == info.keys()
            assert torch.equal(img[..., :3].view(torch.int32), rgb.view(torch.int32)), m
            assert torch.equal(a.view(torch.int32), alpha.view(torch.int32)), m
        for m in ("D", "ED"):
            assert out[m][0].shape == (3, H, W, 1)
            assert torch.equal(out[m][1].view(torch.int32), alpha.view(torch.int32)), m
        D, ED = out["D"][0], out["ED"][0]
        assert torch.equal(D.view(torch.int32), out["RGB+D"][0][..., 3:4].contiguous().view(torch.int32))
        assert torch.equal(ED.view(torch.int32), out["RGB+ED"][0][..., 3:4].contiguous().view(torch.int32))
        np.testing.assert_allclose((ED * alpha.clamp(min=1e-10)).cpu().numpy(), D.cpu().numpy(), rtol=1e-6, atol=0)
        seen = alpha > 0.1
        assert float(D.max()) > 0 and bool(seen.any()) and bool((ED[seen] > 0).all())
        empty = alpha == 0
        assert bool(empty[2].all())
        assert float(D[empty].abs().max()) == 0.0 and float(ED[empty].abs().max()) == 0.0
        assert torch.equal(scene.render_3dgs(w, K, W, H)[0], rgb)
    for bad in ("rgb", "RGBD", "", "D+RGB"):
        with pytest.raises(ValueError):
            scene.render_3dgs(w, K, W, H, render_mode=bad)
    # "RGB" never reaches the new ops
    def boom(*a, **k):
        raise AssertionError("depth op called from an RGB render")
    for fn in ("blend_depth_fwd", "blend_depth_bwd", "depth_bwd"):
        monkeypatch.setattr(ops, fn, boom)
    wg = dev(w2c).requires_grad_()
    rgb2, alpha2, _ = scene.render_3dgs(wg, K, W, H, render_mode="RGB")
    (rgb2.sum() + alpha2.sum()).backward()
    assert torch.equal(rgb2.detach(), rgb) and wg.grad is not None
    with pytest.raises(AssertionError):
        scene.render_3dgs(w, K, W, H, render_mode="D")


def test_render_3dgs_original_takes_render_mode(ctx):
    g, w2c, Ks, W, H = make("small")
    scene = _scene(g)
    scene.intrinsics = dev(Ks)
    scene.c2w = torch.inverse(dev(w2c))
    with torch.no_grad():
        img, alpha, _ = scene.render_3dgs_original(W, H, render_mode="RGB+ED")
        ref, _, _ = scene.render_3dgs(scene.w2c, scene.intrinsics, W, H, render_mode="RGB+ED")
    assert img.shape == (w2c.shape[0], H, W, 4) and torch.equal(img, ref)


# ---- 4. per-pair backward vs oracle ----
def masked_v_depth(meta, shape, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    v[~(meta["margin"] > 1e-4)] = 0.0
    return v


@pytest.mark.parametrize("name", NAMED + FUZZ3)
def test_depth_backward_vs_oracle(ctx, name):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    Cn, N = w2c.shape[0], g["means"].shape[0]
    d_o, alpha_o, meta, zcol = oracle_depth(g, w2c, Ks, W, H)
    v_d = masked_v_depth(meta, d_o.shape)
    v3 = np.zeros(d_o.shape[:3] + (3,), np.float32)
    v3[..., 0] = v_d[..., 0]
    vm, vc, vcol, vo = go.blend_bwd(Cn, W, H, 16, meta["means2d"], meta["conics"], zcol, meta["opacities"],
                                    meta["isect_offsets"], meta["flatten_ids"], alpha_o, meta["last_ids"], v3)
    assert not vcol[:, 1:].any()
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_splats = ops.blend_depth_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                                   info["_last_ids"], dev(v_d), info["_cum_tiles"], Cn, W, H)
    torch.cuda.synchronize()
    assert float(v_splats[:, [6, 7, 8, 10, 11]].abs().max()) == 0.0
    pid = info["camera_ids"].long() * N + info["gaussian_ids"].long()
    vs = v_splats[pid].cpu().numpy()
    hidden = torch.ones(Cn * N, dtype=torch.bool, device="cuda:0"); hidden[pid] = False
    assert float(v_splats[hidden].abs().max()) == 0.0 if bool(hidden.any()) else True
    PAIR_TOL = 2e-4 if name.startswith("fuzz") else 5e-5   # test_gpu_gs.test_backward_vs_oracle
    errs = {}
    for key, a, b in (("v_means2d", vs[:, 0:2], vm), ("v_opacity", vs[:, 2], vo), ("v_conics", vs[:, 3:6], vc),
                      ("v_z", vs[:, 9], vcol[:, 0])):
        errs[key] = float(np.abs(a - b).max() / (np.abs(b).max() + 1e-20))
    print(name, "max error / tensor max:", {k: "%.1e" % v for k, v in errs.items()})
    assert float(np.abs(vcol[:, 0]).max()) > 0
    for key, e in errs.items():
        assert e < PAIR_TOL, (name, key, e)   # measured: regular scenes <= 1.6e-5, fuzz scenes <= 5.7e-5


# ---- 5. st3r_gs_depth_bwd vs float64 ----
def depth_chain_ref(g, w2c, Ks, W, H, splats, vz):
    N, Cn = g["means"].shape[0], w2c.shape[0]
    rad = splats[:, 10].view(torch.int32).reshape(Cn, N).cpu()
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    means = t(g["means"]).requires_grad_()
    quats, scales = t(g["quats"]), t(g["scales"])
    vm = t(w2c).requires_grad_()
    K = t(Ks)
    vz = vz.reshape(Cn, N).double().cpu()
    total = 0.0
    for c in range(Cn):
        idx = torch.nonzero(rad[c] > 0).reshape(-1)
        if idx.numel():
            _, z, _ = tr.project(means[idx], quats[idx], scales[idx], vm[c], K[c], W, H)
            total = total + (z * vz[c, idx]).sum()
    if not torch.is_tensor(total):
        return torch.zeros_like(means), torch.zeros_like(vm)
    gm, gv = torch.autograd.grad(total, (means, vm))
    return gm, gv


@pytest.mark.parametrize("name", NAMED)
def test_depth_bwd_vs_fp64(ctx, name):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    Cn, N = w2c.shape[0], g["means"].shape[0]
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    v_splats = torch.randn((Cn * N, 12), device="cuda:0", generator=_gen(9))
    if Cn > 1:
        v_splats[(Cn - 1) * N:] = 0.0   # the last camera is idle
    gm_ref, gv_ref = depth_chain_ref(g, w2c, Ks, W, H, info["_splats"], v_splats[:, 9])
    grads = torch.zeros(23 * N, device="cuda:0")
    vv = torch.zeros((Cn, 4, 4), device="cuda:0")
    ops.depth_bwd(ctx, P["means"], dev(w2c), info["_splats"], v_splats, grads, vv)
    torch.cuda.synchronize()
    assert float(grads[3 * N:].abs().max()) == 0.0
    gm = grads[:3 * N].view(N, 3)
    e_m = float((gm.double().cpu() - gm_ref).abs().max() / (gm_ref.abs().max() + 1e-30))
    live = Cn - 1 if Cn > 1 else Cn
    e_v = rel_err_per_camera(vv[:live], gv_ref[:live])
    print(name, "means %.1e, viewmats per camera" % e_m, ["%.1e" % e for e in e_v])
    # measured: means <= 9.3e-8, poses <= 4.8e-8
    assert float(gm_ref.abs().max()) > 0 and e_m < 1e-6 and max(e_v) < 1e-6, (name, e_m, e_v)
    assert float(vv[:, [0, 1, 3]].abs().max()) == 0.0      # only row 2 of a pose sees z
    if Cn > 1:
        assert float(vv[Cn - 1].abs().max()) == 0.0 and float(gv_ref[Cn - 1].abs().max()) == 0.0
    # the call ADDS: a second one doubles both outputs exactly; without v_viewmats the means part is the same bits
    first_m, first_v = grads.clone(), vv.clone()
    ops.depth_bwd(ctx, P["means"], dev(w2c), info["_splats"], v_splats, grads, vv)
    only_m = torch.zeros(23 * N, device="cuda:0")
    ops.depth_bwd(ctx, P["means"], dev(w2c), info["_splats"], v_splats, only_m, None)
    torch.cuda.synchronize()
    assert torch.equal(grads, 2 * first_m) and torch.equal(vv, 2 * first_v)
    assert torch.equal(only_m.view(torch.int32), first_m.view(torch.int32))


# ---- 6. end to end vs the float64 dense render ----
def render_dense_depth(means, quats, scales, opacities, sh, viewmats, Ks, W, H, vis_mask, radii, tile_size=16):
    """gs_torch_ref.render_dense with one more output: depth [C,H,W,1] = sum_i w_i z_i, the same weights"""
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


@pytest.mark.parametrize("mode", ["D", "ED", "RGB+ED"])
@pytest.mark.parametrize("name", ["small", "ragged", "one", "many"])
def test_render_depth_grads_vs_dense_fp64(ctx, name, mode):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    Cn, N = w2c.shape[0], g["means"].shape[0]
    _, alpha_o, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"], w2c, Ks, W, H,
                                        want_margin=True)
    ch = 4 if mode.startswith("RGB") else 1
    rng = np.random.default_rng(11)
    v_img = rng.standard_normal((Cn, H, W, ch)).astype(np.float32)
    v_alpha = rng.standard_normal(alpha_o.shape).astype(np.float32)
    und = ~(meta["margin"] > 1e-4)
    v_img[und] = 0.0; v_alpha[und] = 0.0
    if mode.endswith("ED"):
        # the quotient amplifies float32 noise where alpha is small: cotangents of ED only where alpha > 0.05
        thin = ~(alpha_o[..., 0] > 0.05)
        v_img[..., -1][thin] = 0.0
        kept = [float((v_img[c, ..., -1] != 0).mean()) for c in range(Cn)]
        print(name, mode, "share of pixels carrying an ED cotangent per view:", ["%.3f" % k for k in kept])
        assert min(kept) > 0, kept
    scene = _scene(g)
    w = dev(w2c).requires_grad_()
    img, alpha, _ = scene.render_3dgs(w, dev(Ks), W, H, render_mode=mode)
    ((img * dev(v_img)).sum() + (alpha * dev(v_alpha)).sum()).backward()
    info = ops.last_info()
    rad = info["_splats"][:, 10].view(torch.int32).reshape(Cn, N).cpu().to(torch.int64)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    ref = {k: t(g[k]).requires_grad_() for k in ("means", "quats", "scales", "opacities", "shN")}
    vm = t(w2c).requires_grad_()
    rgb_t, alpha_t, d_t = render_dense_depth(ref["means"], ref["quats"], ref["scales"], ref["opacities"], ref["shN"], vm,
                                             t(Ks), W, H, rad > 0, rad)
    if mode.endswith("ED"):
        d_t = d_t / alpha_t.clamp(min=1e-10)
    img_t = torch.cat([rgb_t, d_t], dim=-1) if mode.startswith("RGB") else d_t
    ((img_t * t(v_img)).sum() + (alpha_t * t(v_alpha)).sum()).backward()
    errs = {}
    for k in ("means", "quats", "scales", "opacities", "shN"):
        a, b = scene.gaussians[k].grad.double().cpu(), ref[k].grad
        if b is None:   # a pure depth mode never touches the SH coefficients in the float64 graph
            assert k == "shN" and not mode.startswith("RGB")
            b = torch.zeros_like(ref[k])
        if k == "shN":
            assert float(a[:, 4:].abs().max()) == 0.0
            a, b = a[:, :4], b[:, :4]
        errs[k] = float((a - b).abs().max() / (b.abs().max() + 1e-30))
    if not mode.startswith("RGB"):
        assert float(scene.gaussians["shN"].grad.abs().max()) == 0.0 and ref["shN"].grad is None
    errs["w2c"] = max(rel_err_per_camera(w.grad, vm.grad))
    print(name, mode, "max |d| / max |ref|:", {k: "%.1e" % v for k, v in errs.items()})
    assert float(ref["means"].grad.abs().max()) > 0 and float(vm.grad.abs().max()) > 0
    # measured: <= 1.9e-5 for "D" / "ED"; "RGB+ED" <= 3.0e-5 except shN on `ragged`, 4.8e-5 (the colour backward's own error:
    # the SH gradient takes nothing from the depth channel)
    for k, e in errs.items():
        assert e <= 5e-5, (name, mode, k, e)   # the bar of test_gpu_pose_grad.test_render_w2c_grad_vs_dense_fp64


# ---- 7. nothing else moves; the depth backward is deterministic ----
def test_depth_render_leaves_rgb_gradients_alone_and_is_deterministic(ctx):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make("medium")
    Cn = w2c.shape[0]
    assert Cn >= 2
    scene = _scene(g)
    K = dev(Ks)
    v_rgb = torch.randn((Cn, H, W, 3), device="cuda:0", generator=_gen(1))
    v_d = torch.randn((Cn, H, W, 4), device="cuda:0", generator=_gen(2))

    def backward_of(mode, cot):
        for p in scene.gaussians.values():
            p.grad = None
        w = dev(w2c).requires_grad_()
        img, alpha, _ = scene.render_3dgs(w, K, W, H, render_mode=mode)
        ((img * cot).sum() + alpha.sum()).backward()
        out = {k: p.grad.clone() for k, p in scene.gaussians.items() if p.grad is not None}
        out["w2c"] = w.grad.clone()
        return out

    before = backward_of("RGB", v_rgb)
    d1 = backward_of("RGB+ED", v_d)
    d2 = backward_of("RGB+ED", v_d)
    after = backward_of("RGB", v_rgb)
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
        assert torch.equal(d1[k].view(torch.int32), d2[k].view(torch.int32)), k
        if k != "shN":
            assert not torch.equal(d1[k], before[k]), k
    # the kernel on its own, twice
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    vd = torch.randn(alpha.shape, device="cuda:0", generator=_gen(3))
    a = ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], vd, info["_cum_tiles"], Cn, W, H)
    b = ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], vd, info["_cum_tiles"], Cn, W, H)
    torch.cuda.synchronize()
    assert float(a[:, 9].abs().max()) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 8. the capability ----
def test_pose_recovery_from_depth(ctx):
    """test_gpu_pose_grad.test_pose_recovery with a loss on the expected depth ("ED") ONLY: no colour term."""
    import starst3r_amd as st
    W, H = 160, 120
    g, w2c, Ks = synth.make_scene(20000, 3, W, H, seed=17, scale_lo=0.01, scale_hi=0.08)
    scene = st.Scene(device="cuda:0")
    scene.gaussians = {k: dev(v) for k, v in g.items()}
    w_true = torch.tensor(w2c[1], dtype=torch.float64)
    K1 = dev(Ks[1:2])
    with torch.no_grad():
        gt, _, _ = scene.render_3dgs(dev(w2c[1:2]), K1, W, H, render_mode="ED")
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
        ed, _, _ = scene.render_3dgs(w, K1, W, H, render_mode="ED")
        loss = (ed - gt).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step(); sched.step()
    rot1, tr1 = _pose_errors((_se3_exp(xi) @ w_pert).detach(), w_true)
    print("pose recovery from ED depth alone: rotation %.2e -> %.2e rad (x%.0f), centre %.2e -> %.2e (x%.0f)"
          % (rot0, rot1, rot0 / max(rot1, 1e-30), tr0, tr1, tr0 / max(tr1, 1e-30)))
    # measured: rotation 3.5e-2 -> 1.5e-5 rad, centre 5.4e-2 -> 1.3e-5
    assert rot1 < rot0 / 10 and tr1 < tr0 / 10, (rot0, rot1, tr0, tr1)


# ---- 9. full size ----
def test_depth_full_size_one_view(ctx):
    """SYNTH-1M, one 1920x1080 view, against the depth-as-colour composition of the existing kernels."""
    from starst3r_amd import ops
    W, H = 1920, 1080
    g, w2c, Ks = synth.make_scene(1_000_000, 1, W, H)
    P, rgb, alpha, info = run_hip(ctx, g, w2c, Ks, W, H)
    lists = (info["isect_offsets"], info["_flatten_ids_dense"])
    d = hip_depth(ctx, info, alpha, 1, W, H)
    sz = depth_as_colour(info)
    rgb_z, alpha_z, last_z = ops.blend_fwd(ctx, sz, *lists, 1, W, H)   # (also leaves the masks both backward calls use)
    assert torch.equal(last_z, info["_last_ids"])
    e_fwd = float((d[..., 0] - rgb_z[..., 0]).abs().max() / rgb_z[..., 0].abs().max())
    vd = torch.randn(alpha.shape, device="cuda:0", generator=_gen(6))
    v3 = torch.zeros_like(rgb); v3[..., 0:1] = vd
    ref = ops.blend_bwd(ctx, sz, *lists, alpha, info["_last_ids"], v3, None, info["_cum_tiles"], 1, W, H)
    got = ops.blend_depth_bwd(ctx, info["_splats"], *lists, alpha, info["_last_ids"], vd, info["_cum_tiles"], 1, W, H)
    torch.cuda.synchronize()
    e_z = float((got[:, 9] - ref[:, 6]).abs().max() / ref[:, 6].abs().max())
    print("SYNTH-1M one view: D %.1e, v_z %.1e of max" % (e_fwd, e_z))
    assert float(d.max()) > 0 and float(ref[:, 6].abs().max()) > 0
    assert e_fwd <= 1e-4 and e_z <= 1e-4, (e_fwd, e_z)   # measured: 0 and 0
