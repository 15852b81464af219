"""Per-step time of the benchmark's size with nothing registered, with backgrounds, and with backgrounds and alpha targets
(profiles/alpha_step.md), the blend backward's stage time in each setting, and the two streaming kernels on their own.

    python tools/time_alpha_step.py [--n 1000000] [--views 8] [--steps 60] [--reps 50]

Alternates blocks of steps of the three settings in one process (same clocks, same allocator state, same scene) and prints
median / min / max of each from HIP events around whole steps.  The run without a registration executes the launches of a
build without the feature.  Then the same settings once more with the library's per-stage events on (st3r_ctx_set_profiling):
the loss stage, which holds the composite and st3r_alpha_grad, and the blend backward, which takes k_blend_bwd<true> as soon
as a v_alpha exists.  Then st3r_composite_fwd and st3r_alpha_grad on the step's images, HIP events around every launch, with
the bytes they have to move."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from st3r_synth import synth   # noqa: E402
from starst3r_amd import ops   # noqa: E402

SETTINGS = ("off", "backgrounds", "backgrounds + alpha targets")


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
    rgb, alpha, _ = ops.render(ctx, P, vm, K, campos, W, H)
    # white backgrounds; the photographs are the render over them and the targets the render's own alpha perturbed, with a
    # third of the weights zero
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    b = torch.ones((C, 3), device="cuda:0")
    gt = ops.composite_fwd(ctx, rgb, alpha, b).contiguous()
    M = torch.clamp(alpha[..., 0] + 0.1 * torch.randn(alpha.shape[:3], device="cuda:0", generator=gen), 0, 1).contiguous()
    wt = (torch.rand(M.shape, device="cuda:0", generator=gen) > 0.33).float().contiguous()
    N = a.n
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))

    def register(setting):
        ops.set_background(ctx, gt, b) if setting != "off" else ops.set_background(ctx, None, None)
        ops.set_alpha_target(ctx, gt, M, wt, 1.0) if setting == SETTINGS[2] else ops.set_alpha_target(ctx, None, None, None)

    step = [0]

    def one_step():
        step[0] += 1
        ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8, step[0], loss,
                       want_stats=False)

    times = {s: [] for s in SETTINGS}
    per_block = max(4, a.steps // 3)
    for block in range(9):
        setting = SETTINGS[block % 3]
        register(setting)
        for it in range(per_block):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one_step()
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first steps of a block size their buffers and compute the registration's normalisers
                times[setting].append(e0.elapsed_time(e1))
    ops.settle(ctx)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}")
    for s in SETTINGS:
        t = np.array(times[s])
        print("%-28s median %.3f ms, min %.3f, max %.3f over %d steps" % (s + ":", np.median(t), t.min(), t.max(), t.size))
    # the stages, per setting, from the library's own events
    print("stage times from st3r_ctx_set_profiling, ms per step (mean over %d steps)" % (per_block - 3))
    for s in SETTINGS:
        register(s)
        for it in range(3):
            one_step()
        ops.settle(ctx)
        ops.set_profiling(ctx, True)
        ops.stage_ms(ctx)
        for it in range(per_block - 3):
            one_step()
        ms = ops.stage_ms(ctx)
        ops.set_profiling(ctx, False)
        print("%-28s " % (s + ":") + ", ".join("%s %.3f" % (k, ms[k][0] / max(ms[k][1], 1))
                                                for k in ("blend_fwd", "loss", "blend_bwd", "project_bwd")))
    ops.settle(ctx)
    register("off")
    # the two kernels on their own
    v_y = torch.randn(rgb.shape, device="cuda:0", generator=gen)
    v_in = torch.randn(alpha.shape, device="cuda:0", generator=gen)
    y = torch.empty_like(rgb); v_a = torch.empty_like(alpha)
    px = C * H * W
    cases = {
        "composite_fwd": (lambda: ops.composite_fwd(ctx, rgb, alpha, b, out=y), 28 * px),
        "alpha_grad background": (lambda: ops.alpha_grad(ctx, alpha, b, v_y, v_alpha=v_a), 20 * px),
        "alpha_grad alpha": (lambda: ops.alpha_grad(ctx, alpha, target=M, weight=wt, alpha_fac=1.0, v_alpha=v_a), 16 * px),
        "alpha_grad both": (lambda: ops.alpha_grad(ctx, alpha, b, v_y, M, wt, 1.0, v_alpha=v_a), 28 * px),
        "alpha_grad both, accumulate": (lambda: ops.alpha_grad(ctx, alpha, b, v_y, M, wt, 1.0, v_alpha_in=v_in, v_alpha=v_a),
                                        32 * px),
    }
    ms = {k: [] for k in cases}
    for rep in range(-5, a.reps):   # negative: warm-up
        for name, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
    print(f"stage kernels, {C} x {W}x{H} = {px / 1e6:.1f} Mpx, {a.reps} calls each (median / min ms, bytes moved, GB/s at the median);")
    print("the alpha-term calls include the weights' normaliser launches (k_weight_sums + k_stream_finish: 4 B per pixel more),")
    print("which a registered step runs once per registration, and every call with a sum its finishing launch")
    for name, (_, nbytes) in cases.items():
        med = float(np.median(ms[name]))
        print(f"  {name:30s} {med:8.3f} {min(ms[name]):8.3f} {nbytes / 1e6:8.1f} MB {nbytes / med / 1e6:8.0f}")


if __name__ == "__main__":
    main()
