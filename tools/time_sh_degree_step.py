"""Per-step time of the benchmark's size at SH degree 1 and at degree 3 (profiles/sh_degree_step.md).

    python tools/time_sh_degree_step.py [--n 1000000] [--views 8] [--steps 20] [--rounds 8]

Alternates blocks of steps of the two settings in one process, the order reversed every round (same build, same clocks, same
allocator state), and prints per setting the mean of the rounds' medians with its standard error, the paired difference by
round, and the spread of a setting's own rounds, from HIP events around whole steps.  Degree 1 is the context's default
(st3r_gs_train_step on a compact [N, 4, 3] SH copy: the launches of a build without the feature); degree 3 is
st3r_ctx_set_sh_degree(ctx, 3, 3, v_sh_high) on a compact [N, 16, 3] copy of the same scene with random rows 1..15, followed by
st3r_sh_high_adam_step.  Learning rates 0: the scene stays the same.  Then the stage times (st3r_ctx_set_profiling) of
projection, projection backward and Adam of one block per setting."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    W, H, C, N = a.width, a.height, a.views, a.n
    ctx = ops.Context("cuda:0")
    g, w2c, Ks = synth.make_scene(N, C, W, H)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda:0")
    P = {k: dev(v) for k, v in g.items()}
    sh16 = P["shN"][:, :16].contiguous()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    sh16[:, 4:] = 0.1 * (2 * torch.rand((N, 12, 3), device="cuda:0", generator=gen) - 1)
    P1 = dict(P, shN=sh16[:, :4].contiguous())
    P3 = dict(P, shN=sh16)
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(ctx, P1, vm, K, campos, W, H)
    gt = rgb.clamp(0, 1).contiguous()
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    hi = torch.zeros((N, 36), device="cuda:0"); hm = torch.zeros_like(hi); hv = torch.zeros_like(hi)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))
    step = [0]

    def one_step(deg):
        step[0] += 1
        ops.train_step(ctx, P3 if deg == 3 else P1, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999,
                       1e-8, step[0], loss, want_stats=False)
        if deg == 3:
            ops.sh_high_adam_step(ctx, sh16, 3, hi, hm, hv, 0.0, 0.9, 0.999, 1e-8, step[0])

    def setting(deg):
        if deg == 3:
            ops.set_sh_degree(ctx, 3, 3, hi)
        else:
            ops.set_sh_degree(ctx, *ops.SH_DEFAULT)

    med = {1: [], 3: []}
    for r in range(a.rounds):
        for deg in ((1, 3) if r % 2 == 0 else (3, 1)):
            setting(deg)
            t = []
            for it in range(a.steps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                one_step(deg)
                e1.record()
                e1.synchronize()
                if it >= 3:   # the first steps of a block size their buffers
                    t.append(e0.elapsed_time(e1))
            ops.settle(ctx)
            med[deg].append(float(np.median(t)))
    se = lambda x: float(np.std(x) / max(len(x) - 1, 1) ** 0.5)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}, {a.rounds} rounds of {a.steps} steps per setting (medians per round, ms)")
    for deg in (1, 3):
        x = np.array(med[deg])
        print("degree %d: mean %.4f +- %.4f, spread of its rounds %.4f: %s"
              % (deg, x.mean(), se(x), x.max() - x.min(), " ".join("%.4f" % e for e in x)))
    d = np.array(med[3]) - np.array(med[1])
    print("degree 3 minus degree 1, paired by round: %+.4f +- %.4f ms" % (d.mean(), se(d)))
    # stage times of one block per setting
    for deg in (1, 3):
        setting(deg)
        ops.set_profiling(ctx, True)
        for it in range(a.steps + 3):
            one_step(deg)
        ops.settle(ctx)
        torch.cuda.synchronize()
        ms = ops.stage_ms(ctx)
        ops.set_profiling(ctx, False)
        print("degree %d stages, mean ms (the 23-float Adam only; the high block's launch is not a stage): " % deg +
              ", ".join("%s %.4f" % (k, ms[k][0] / max(ms[k][1], 1)) for k in ("project", "project_bwd", "adam")))
    setting(1)


if __name__ == "__main__":
    main()
