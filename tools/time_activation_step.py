"""Per-step time of the benchmark's size with the activation off and on (profiles/activation_step.md), and the two streaming
kernels of csrc/gs_activation.hip on their own.

    python tools/time_activation_step.py [--n 1000000] [--views 8] [--steps 20] [--rounds 8] [--reps 50]

Alternates blocks of steps of the two settings in one process, the order reversed every round (same build, same clocks, same
allocator state), and prints per setting the mean of the rounds' medians with its standard error, the paired difference by
round, and the spread of a setting's own rounds, from HIP events around whole steps.  Both settings render the same scene:
off gets scales s and opacities o (clamped to 0.999), on gets log(s) and logit(o).  The run with the setting off executes the
launches of a build without the feature.  Then st3r_param_activate (with and without its sums) and st3r_param_activate_bwd
(out of place and in place), HIP events around every call, with the bytes they have to move."""
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
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    W, H, C, N = a.width, a.height, a.views, a.n
    ctx = ops.Context("cuda:0")
    g, w2c, Ks = synth.make_scene(N, C, W, H)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda:0")
    g["opacities"] = np.minimum(g["opacities"], np.float32(0.999))
    P = {k: dev(v) for k, v in g.items()}
    P["shN"] = P["shN"][:, :4].contiguous()
    o64 = g["opacities"].astype(np.float64)
    PL = dict(P, scales=dev(np.log(g["scales"].astype(np.float64))), opacities=dev(np.log(o64) - np.log1p(-o64)))
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(ctx, P, vm, K, campos, W, H)
    gt = rgb.clamp(0, 1).contiguous()
    grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
    loss = torch.zeros(1, device="cuda:0")
    ops.set_gt_moments(ctx, gt, ops.gt_moments(ctx, gt))
    step = [0]

    def one_step(on):
        step[0] += 1
        ops.train_step(ctx, PL if on else P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 0.0, 0.9, 0.999, 1e-8,
                       step[0], loss, want_stats=False)

    med = {False: [], True: []}
    for r in range(a.rounds):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            ops.set_activation(ctx, on)
            t = []
            for it in range(a.steps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                one_step(on)
                e1.record()
                e1.synchronize()
                if it >= 3:   # the first steps of a block size their buffers
                    t.append(e0.elapsed_time(e1))
            ops.settle(ctx)
            med[on].append(float(np.median(t)))
    ops.set_activation(ctx, False)
    se = lambda x: float(np.std(x) / max(len(x) - 1, 1) ** 0.5)
    print(f"fused step, {N} Gaussians, {C} x {W}x{H}, {a.rounds} rounds of {a.steps} steps per setting (medians per round, ms)")
    for on in (False, True):
        x = np.array(med[on])
        print("activation %-4s mean %.4f +- %.4f, spread of its rounds %.4f: %s"
              % ("on:" if on else "off:", x.mean(), se(x), x.max() - x.min(), " ".join("%.4f" % e for e in x)))
    d = np.array(med[True]) - np.array(med[False])
    print("on minus off, paired by round: %+.4f +- %.4f ms" % (d.mean(), se(d)))
    # the two kernels on their own
    S, O, _ = ops.param_activate(ctx, PL["scales"], PL["opacities"])
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    v_S = torch.randn(S.shape, device="cuda:0", generator=gen); v_O = torch.randn(O.shape, device="cuda:0", generator=gen)
    o_S, o_O = torch.empty_like(S), torch.empty_like(O)
    cases = {
        "param_activate": (lambda: ops.param_activate(ctx, PL["scales"], PL["opacities"], S, O), 32 * N),
        "param_activate, sums": (lambda: ops.param_activate(ctx, PL["scales"], PL["opacities"], S, O, want_sums=True), 32 * N),
        "param_activate_bwd": (lambda: ops.param_activate_bwd(ctx, S, O, v_S, v_O, 1e-8, 1e-8, o_S, o_O), 48 * N),
        "param_activate_bwd, in place": (lambda: ops.param_activate_bwd(ctx, S, O, v_S, v_O, 0.0, 0.0, v_S, v_O), 48 * N),
    }
    ms = {k: [] for k in cases}
    for rep in range(-5, a.reps):   # negative: warm-up
        for name, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
    print(f"kernels, {N} Gaussians, {a.reps} calls each (median / min ms, bytes moved, GB/s at the median); the call with the")
    print("sums includes its finishing launch and the allocation of the result")
    for name, (_, nbytes) in cases.items():
        md = float(np.median(ms[name]))
        print(f"  {name:30s} {md:8.4f} {min(ms[name]):8.4f} {nbytes / 1e6:8.1f} MB {nbytes / md / 1e6:8.0f}")


if __name__ == "__main__":
    main()
