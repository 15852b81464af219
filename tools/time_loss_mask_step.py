"""Per-step time of the benchmark's size with and without per-pixel loss weights registered (profiles/loss_mask_step.md),
and the weighted and unweighted loss launches on their own.

    python tools/time_loss_mask_step.py [--n 1000000] [--views 8] [--steps 60] [--reps 50]

Alternates blocks of steps with the registration off and on in one process (same clocks, same allocator state, same
scene) and prints the median, minimum and maximum step time of each from HIP events around whole steps.  The run without
a registration executes the launches of a build without the feature.  The ground-truth moments are registered throughout,
as run_3dgs_optim registers them.  Then st3r_loss_l1_ssim and st3r_loss_l1_ssim_weighted on the step's images, with and
without registered moments, HIP events around every call (the weighted call includes its normaliser launches, which a
registered step runs once per registration only)."""
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
    W, H, C = a.width, a.height, a.views
    ctx = ops.Context("cuda:0")
    g, w2c, Ks = synth.make_scene(a.n, C, W, H)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda:0")
    P = {k: dev(v) for k, v in g.items()}
    P["shN"] = P["shN"][:, :4].contiguous()
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(ctx, P, vm, K, campos, W, H)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    gt = torch.clamp(rgb + 0.05 * torch.randn(rgb.shape, device="cuda:0", generator=gen), 0, 1).contiguous()
    # a confidence-like map with a dropped rectangle per view
    wgt = torch.rand((C, H, W), device="cuda:0", generator=gen) * 2.0
    wgt[:, H // 4:H // 2, W // 3:2 * W // 3] = 0.0
    wgt = wgt.contiguous()
    N = a.n
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    mom = ops.gt_moments(ctx, gt)
    ops.set_gt_moments(ctx, gt, mom)
    times = {False: [], True: []}
    step = 0
    for block in range(6):
        on = bool(block % 2)
        ops.set_loss_weight(ctx, gt, wgt) if on else ops.set_loss_weight(ctx, None, None)
        for it in range(a.steps // 3):
            step += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8, step, loss,
                           want_stats=False)
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first steps of a block size their buffers (and compute the registration's normalisers)
                times[on].append(e0.elapsed_time(e1))
    ops.settle(ctx)
    ops.set_loss_weight(ctx, None, None)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}")
    for on in (False, True):
        t = np.array(times[on])
        print("loss weights %s: median %.3f ms, min %.3f, max %.3f over %d steps" % ("on " if on else "off", np.median(t),
                                                                                      t.min(), t.max(), t.size))
    # the loss launches on their own
    cases = {"loss_l1_ssim": lambda: ops.loss_l1_ssim(ctx, rgb, gt, 0.8, 0.2),
             "loss_l1_ssim_weighted": lambda: ops.loss_l1_ssim_weighted(ctx, rgb, gt, wgt, 0.8, 0.2)}
    px = C * H * W
    print(f"loss launches, {C} x {W}x{H} = {px / 1e6:.1f} Mpx, {a.reps} calls each (median / min / max ms)")
    for moments in (True, False):
        ops.set_gt_moments(ctx, gt, mom) if moments else ops.set_gt_moments(ctx, None, None)
        ms = {k: [] for k in cases}
        for rep in range(-5, a.reps):   # negative: warm-up
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep >= 0:
                    ms[name].append(e0.elapsed_time(e1))
        for name in cases:
            t = np.array(ms[name])
            print(f"  {name:24s} moments {'registered' if moments else 'not registered'}: {np.median(t):8.3f} {t.min():8.3f} "
                  f"{t.max():8.3f}")
    ops.set_gt_moments(ctx, None, None)


if __name__ == "__main__":
    main()
