"""Every output array of the fused 3DGS step under each of its options, saved for a bit comparison between two builds: the
gate "same bits" of a refactor of the step's host side (profiles/step_options_refactor.md).

    python tools/step_options_bits.py out.npz            # in the parent's tree (twice) and in the tree under review
    python tools/step_options_bits.py --compare a.npz b.npz [c.npz]

Scenes: N = 300, V = 3, 40 x 24 (tests/test_gpu_view_registration.py) and "small" of tests/per_view_cases.py.  Settings:
nothing, each of the six registrations alone, all six together, the activation, SH degree 3 -- each whole and under debug
flag 32 (two view chunks).  Per setting: train_fwd_bwd, three train_step, three train_step_poses; saved: grads, parameters,
moments, losses, v_exposure, v_Ks, v_viewmats, the poses and their moments, v_sh_high.  Then st3r_gs_raster_train and
st3r_gs_render.  --compare: np.array_equal on the integer views of a and b; with c (a second run of a's build), an array
that differs between a and c may differ between a and b by at most as much."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B1, B2, EPS = 0.9, 0.999, 1e-8
REGISTRATIONS = ("depth_prior", "exposure", "intrinsics_grad", "loss_weight", "background", "alpha_target")
SETTINGS = ("none",) + REGISTRATIONS + ("all_six", "activation", "sh_degree_3")


def scenes():
    from st3r_synth import synth
    from per_view_cases import make
    g, w2c, Ks = synth.make_scene(300, 3, 40, 24, seed=7, scale_lo=0.02, scale_hi=0.08)
    yield "n300", g, w2c, Ks, 40, 24
    g, w2c, Ks, W, H = make("small")
    yield "small", g, w2c, Ks, W, H


def run_scene(out, name, g, w2c, Ks, W, H):
    from starst3r_amd import ops
    from per_view_cases import _setup, _synthetic_prior
    ctx = ops.Context("cuda:0")
    rng = np.random.default_rng(3)
    g["shN"][:, 4:16, :] = rng.uniform(-0.1, 0.1, (g["shN"].shape[0], 12, 3)).astype(np.float32)
    P0, vm0, K, campos0, gt = _setup(ctx, g, w2c, Ks, W, H)
    N, V = P0["means"].shape[0], vm0.shape[0]
    Z, wt, info = _synthetic_prior(ctx, P0, vm0, K, W, H)
    gen = torch.Generator().manual_seed(11)
    E = (torch.eye(3, 4) + 0.1 * torch.randn((V, 3, 4), generator=gen)).cuda()
    lw = torch.rand((V, H, W), generator=gen)
    lw[torch.rand((V, H, W), generator=gen) < 0.3] = 0.0
    bg = torch.rand((V, 3), generator=gen).cuda()
    M, aw = torch.rand((V, H, W), generator=gen).cuda(), (torch.rand((V, H, W), generator=gen) > 0.3).float().cuda()
    lw = lw.cuda()
    vE, vK = torch.zeros((V, 3, 4), device="cuda:0"), torch.zeros((V, 4), device="cuda:0")
    # log-scales and logits for the activation
    PA = dict(P0, scales=torch.log(P0["scales"].abs().clamp(min=1e-4)).contiguous())
    o = P0["opacities"].clamp(0.05, 0.95)
    PA["opacities"] = torch.log(o / (1 - o)).contiguous()
    hi = torch.zeros((N, 36), device="cuda:0")

    def register(setting, on):
        both = setting == "all_six"
        if both or setting == "depth_prior":
            ops.set_depth_prior(ctx, gt, Z, wt, 0.5) if on else ops.set_depth_prior(ctx, None, None, None)
        if both or setting == "exposure":
            ops.set_exposure(ctx, gt, E, vE) if on else ops.set_exposure(ctx, None, None, None)
        if both or setting == "intrinsics_grad":
            ops.set_intrinsics_grad(ctx, gt, vK) if on else ops.set_intrinsics_grad(ctx, None, None)
        if both or setting == "loss_weight":
            ops.set_loss_weight(ctx, gt, lw) if on else ops.set_loss_weight(ctx, None, None)
        if both or setting == "background":
            ops.set_background(ctx, gt, bg) if on else ops.set_background(ctx, None, None)
        if both or setting == "alpha_target":
            ops.set_alpha_target(ctx, gt, M, aw, 0.5) if on else ops.set_alpha_target(ctx, None, None, None)
        if setting == "activation":
            ops.set_activation(ctx, on)
        if setting == "sh_degree_3":
            ops.set_sh_degree(ctx, 3, 3, hi) if on else ops.set_sh_degree(ctx, *ops.SH_DEFAULT)

    def save(tag, **arrays):
        torch.cuda.synchronize()
        for k, t in arrays.items():
            out[f"{name}/{tag}/{k}"] = t.detach().cpu().numpy().copy()

    for setting in SETTINGS:
        for debug in (0, 32):
            tag = f"{setting}/chunks{1 + debug // 32}"
            start = PA if setting == "activation" else P0
            register(setting, True)
            ops.set_debug(ctx, debug)
            try:
                vE.fill_(-1.0); vK.fill_(-1.0); hi.fill_(-1.0)
                grads, loss = torch.full((23 * N,), -1.0, device="cuda:0"), torch.zeros(7, device="cuda:0")
                ops.train_fwd_bwd(ctx, start, vm0, K, campos0, gt, W, H, 0.2, 0.01, 0.01, grads, loss[0:1])
                save(tag + "/train_fwd_bwd", grads=grads, vE=vE, vK=vK, hi=hi)
                P = {k: v.clone() for k, v in start.items()}
                m, v = torch.zeros_like(grads), torch.zeros_like(grads)
                for it in range(3):
                    ops.train_step(ctx, P, vm0, K, campos0, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, it + 1,
                                   loss[1 + it:2 + it])
                ops.settle(ctx)
                save(tag + "/train_step", grads=grads, m=m, v=v, vE=vE, vK=vK, hi=hi, **P)
                P = {k: v.clone() for k, v in start.items()}
                vm, campos = vm0.clone(), campos0.clone()
                m, v = torch.zeros_like(grads), torch.zeros_like(grads)
                pm, pv, vvm = torch.zeros(6 * V, device="cuda:0"), torch.zeros(6 * V, device="cuda:0"), torch.zeros_like(vm)
                for it in range(3):
                    ops.train_step_poses(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS,
                                         it + 1, loss[4 + it:5 + it], pm, pv, 1e-3, it + 1, None, vvm)
                ops.settle(ctx)
                save(tag + "/train_step_poses", grads=grads, m=m, v=v, vE=vE, vK=vK, hi=hi, vm=vm, campos=campos, pm=pm, pv=pv,
                     v_viewmats=vvm, loss=loss, **P)
            finally:
                ops.set_debug(ctx, 0)
                register(setting, False)
    records = info["_splats"].reshape(-1, 12).contiguous()
    v_rec, loss = torch.full((V * N, 12), -1.0, device="cuda:0"), torch.zeros(1, device="cuda:0")
    ops.raster_train(ctx, records, N, V, gt, W, H, 0.2, v_rec, loss)
    save("raster_train", v_records=v_rec, loss=loss)
    rgb, alpha, _ = ops.render(ctx, P0, vm0, K, campos0, W, H)
    save("render", rgb=rgb, alpha=alpha)
    ctx.close()


def as_int(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def compare(paths):
    a, b = np.load(paths[0]), np.load(paths[1])
    c = np.load(paths[2]) if len(paths) > 2 else None
    assert sorted(a.files) == sorted(b.files), "the two runs saved different arrays"
    differ, noisy, over = [], [], []
    for k in a.files:
        if c is not None and not np.array_equal(as_int(a[k]), as_int(c[k])):
            noisy.append(k)
        if not np.array_equal(as_int(a[k]), as_int(b[k])):
            differ.append(k)
            own = np.abs(a[k].astype(np.float64) - c[k].astype(np.float64)).max() if k in noisy else 0.0
            if not np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max() <= own:
                over.append(k)
    print(f"{len(a.files)} arrays; {len(a.files) - len(differ)} with equal bits in {paths[0]} and {paths[1]}")
    if c is not None:
        print(f"{len(noisy)} differ between {paths[0]} and its own repeat {paths[2]}:", *noisy, sep="\n  ")
    print(f"{len(differ)} differ between the two builds:", *differ, sep="\n  ")
    print(f"{len(over)} differ by more than the first build's own repeat:", *over, sep="\n  ")
    return 1 if over else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    assert torch.cuda.is_available()
    out = {}
    for scene in scenes():
        run_scene(out, *scene)
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
