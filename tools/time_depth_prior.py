"""Per-step time of the benchmark's size with and without a depth prior registered (profiles/depth_prior_step.md).

    python tools/time_depth_prior.py [--n 1000000] [--views 8] [--steps 60]

Alternates blocks of steps with the prior off and on in one process (same clocks, same allocator state) and prints the
median step time of each from HIP events around whole steps."""
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
    a = ap.parse_args()
    W, H = a.width, a.height
    ctx = ops.Context("cuda:0")
    g, w2c, Ks = synth.make_scene(a.n, a.views, W, H)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda:0")
    P = {k: dev(v) for k, v in g.items()}
    P["shN"] = P["shN"][:, :4].contiguous()
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    gt, alpha, _ = ops.render(ctx, P, vm, K, campos, W, H)
    gt = gt.contiguous()
    Z = torch.full((a.views, H, W), 3.5, device="cuda:0")
    wt = (alpha[..., 0] > 0.5).float().contiguous()
    N = a.n
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))
    times = {False: [], True: []}
    step = 0
    for block in range(6):
        on = bool(block % 2)
        ops.set_depth_prior(ctx, gt, Z, wt, 1.0) if on else ops.set_depth_prior(ctx, None, None, None)
        for it in range(a.steps // 3):
            step += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8, step, loss,
                           want_stats=False)
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first steps of a block size their buffers
                times[on].append(e0.elapsed_time(e1))
    ops.settle(ctx)
    for on in (False, True):
        t = np.array(times[on])
        print("prior %s: median %.3f ms, min %.3f, max %.3f over %d steps" % ("on " if on else "off", np.median(t), t.min(),
                                                                               t.max(), t.size))


if __name__ == "__main__":
    main()
