"""Per-step time of the benchmark's size with and without exposures registered (profiles/exposure_step.md), and the two
streaming kernels on their own.

    python tools/time_exposure_step.py [--n 1000000] [--views 8] [--steps 60] [--reps 50]

Alternates blocks of steps with the registration off and on in one process (same clocks, same allocator state, same
scene) and prints the median step time of each from HIP events around whole steps; the registered steps include the
exposure Adam launch.  The run without a registration executes the launches of a build without the feature.  Then
st3r_exposure_fwd and st3r_exposure_bwd on the step's images, HIP events around every launch, with the bytes they move."""
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
    # exposures near the identity; the photographs are the render through them, so the loss is the same in both settings
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    E = torch.eye(3, 4, device="cuda:0").repeat(C, 1, 1) + 0.05 * torch.randn((C, 3, 4), device="cuda:0", generator=gen)
    E = E.contiguous()
    vE = torch.zeros_like(E); em = torch.zeros(12 * C, device="cuda:0"); ev = torch.zeros_like(em)
    gt = rgb.contiguous()
    N = a.n
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))
    times = {False: [], True: []}
    step = 0
    for block in range(6):
        on = bool(block % 2)
        ops.set_exposure(ctx, gt, E, vE) if on else ops.set_exposure(ctx, None, None, None)
        for it in range(a.steps // 3):
            step += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8, step, loss,
                           want_stats=False)
            if on:   # rate 0: the scene stays the same
                ops.exposure_adam_step(ctx, E, vE, em, ev, 0.0, 0.9, 0.999, 1e-8, step)
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first steps of a block size their buffers
                times[on].append(e0.elapsed_time(e1))
    ops.settle(ctx)
    ops.set_exposure(ctx, None, None, None)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}")
    for on in (False, True):
        t = np.array(times[on])
        print("exposures %s: median %.3f ms, min %.3f, max %.3f over %d steps" % ("on " if on else "off", np.median(t), t.min(),
                                                                                   t.max(), t.size))
    # the two kernels on their own
    v_y = torch.randn(rgb.shape, device="cuda:0", generator=gen)
    y = torch.empty_like(rgb); v_x = torch.empty_like(rgb)
    px = C * H * W
    cases = {"exposure_fwd": (lambda: ops.exposure_fwd(ctx, rgb, E, out=y), 24 * px),
             "exposure_bwd": (lambda: ops.exposure_bwd(ctx, rgb, E, v_y, v_rgb=v_x, v_exposure=vE), 36 * px),
             "exposure_bwd in place": (lambda: ops.exposure_bwd(ctx, rgb, E, v_y, v_rgb=v_y, v_exposure=vE), 36 * px)}
    ms = {k: [] for k in cases}
    for rep in range(-5, a.reps):   # negative: warm-up
        for name, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
    print(f"stage kernels, {C} x {W}x{H} = {px / 1e6:.1f} Mpx, {a.reps} launches each (median / min ms, bytes moved, GB/s at the median)")
    for name, (_, nbytes) in cases.items():
        med = float(np.median(ms[name]))
        print(f"  {name:24s} {med:8.3f} {min(ms[name]):8.3f} {nbytes / 1e6:8.1f} MB {nbytes / med / 1e6:8.0f}")


if __name__ == "__main__":
    main()
