"""Per-step time of the benchmark's size with and without an intrinsics gradient registered
(profiles/intrinsics_step.md), and the stand-alone intrinsics backward beside the pose backward.

    python tools/time_intrinsics_step.py [--n 1000000] [--views 8] [--steps 60] [--reps 50]

Alternates blocks of steps with the registration off and on in one process (same clocks, same allocator state, same
scene) and prints the median step time of each from HIP events around whole steps; the registered steps include the
intrinsics Adam launch (rate 0: the scene stays the same).  The run without a registration executes the launches of a
build without the feature.  Then st3r_gs_intrinsics_bwd and st3r_gs_viewmat_bwd on the per-pair gradients of the same
scene, alternating, HIP events around every call."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from st3r_synth import synth   # noqa: E402
from starst3r_amd import ops   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    W, H, C, N = a.width, a.height, a.views, a.n
    ctx = ops.Context("cuda:0")
    g, w2c, Ks = synth.make_scene(N, C, W, H)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda:0")
    P = {k: dev(v) for k, v in g.items()}
    P["shN"] = P["shN"][:, :4].contiguous()   # the compact SH rows run_3dgs_optim trains
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    gt, _, _ = ops.render(ctx, {k: dev(v) for k, v in synth.perturb_for_gt(g).items()}, vm, K, campos, W, H)
    gt = gt.contiguous()
    vK = torch.zeros((C, 4), device="cuda:0"); km = torch.zeros(4 * C, device="cuda:0"); kv = torch.zeros_like(km)
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))
    times = {False: [], True: []}
    step = 0
    for block in range(6):
        on = bool(block % 2)
        ops.set_intrinsics_grad(ctx, gt, vK) if on else ops.set_intrinsics_grad(ctx, None, None)
        for it in range(a.steps // 3):
            step += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8, step, loss,
                           want_stats=False)
            if on:
                ops.intrinsics_adam_step(ctx, K, vK, km, kv, 0.0, 0.9, 0.999, 1e-8, step, None, W, H)
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first steps of a block size their buffers
                times[on].append(e0.elapsed_time(e1))
    ops.settle(ctx)
    ops.set_intrinsics_grad(ctx, None, None)
    ops.set_gt_moments(ctx, None, None)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}")
    for on in (False, True):
        t = np.array(times[on])
        print("intrinsics gradient %s: median %.3f ms, min %.3f, max %.3f over %d steps"
              % ("on " if on else "off", np.median(t), t.min(), t.max(), t.size))
    print("v_Ks of the last registered step (fx, fy, cx, cy per view):", vK.cpu().numpy().round(6).tolist()[:2], "...")
    # the two per-pair reductions on their own
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
    _, v_rgb = ops.loss_l1_ssim(ctx, rgb, gt, 0.8, 0.2)
    v_splats = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_rgb, None, info["_cum_tiles"], C, W, H)
    n_vis = int((info["_splats"][:, 10].view(torch.int32) > 0).sum())
    out_k = torch.empty((C, 4), device="cuda:0"); out_v = torch.empty((C, 4, 4), device="cuda:0")
    cases = {"st3r_gs_intrinsics_bwd": lambda: ops.intrinsics_bwd(ctx, P["means"], P["quats"], P["scales"], vm, K, W, H,
                                                                  info["_splats"], v_splats, out=out_k),
             "st3r_gs_viewmat_bwd": lambda: ops.viewmat_bwd(ctx, P["means"], P["quats"], P["scales"], P["shN"], vm, K,
                                                            info["_campos"], W, H, info["_splats"], v_splats, out=out_v)}
    ms = {k: [] for k in cases}
    for rep in range(-5, a.reps):   # negative: warm-up
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
    print(f"stand-alone, {N * C} pairs of which {n_vis} visible, {a.reps} calls each, alternating (median / min / max ms)")
    for name in cases:
        print(f"  {name:24s} {float(np.median(ms[name])):8.3f} {min(ms[name]):8.3f} {max(ms[name]):8.3f}")


if __name__ == "__main__":
    main()
