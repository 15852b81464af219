"""Times the depth blend kernels against the three-channel kernels they parallel, at SYNTH-1M, 8 x 1080p:
  (i)  blend_depth_fwd  against  blend_fwd on the same lists;
  (ii) blend_depth_bwd  against  blend_bwd fed depth-as-colour (what a user could do before: a record copy whose colour
       is (z, 0, 0), copy included).
HIP events around every launch, old and new alternating in one process, medians over REPS launches after warm-up.
    python tools/time_depth.py [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from starst3r_amd import ops
from st3r_synth import synth

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
N, V, W, H = 1_000_000, 8, 1920, 1080
g, w2c, Ks = synth.make_scene(N, V, W, H)
dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda:0")
P = {k: dev(v) for k, v in g.items()}
ctx = ops.get_context("cuda:0")
rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], dev(w2c), dev(Ks),
                                     W, H)
splats, off, flat = info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"]
last, cum = info["_last_ids"], info["_cum_tiles"]
gen = torch.Generator(device="cuda:0").manual_seed(0)
v_d = torch.randn(alpha.shape, device="cuda:0", generator=gen)
v_3 = torch.zeros_like(rgb); v_3[..., 0:1] = v_d


def colour_bwd_on_depth():
    s = splats.clone()
    s[:, 6] = s[:, 9]; s[:, 7:9] = 0.0
    return ops.blend_bwd(ctx, s, off, flat, alpha, last, v_3, None, cum, V, W, H)


CASES = {
    "blend_fwd (3 channels)": lambda: ops.blend_fwd(ctx, splats, off, flat, V, W, H),
    "blend_depth_fwd": lambda: ops.blend_depth_fwd(ctx, splats, off, flat, alpha, last, V, W, H),
    "blend_bwd on depth-as-colour (with the record copy)": colour_bwd_on_depth,
    "blend_depth_bwd": lambda: ops.blend_depth_bwd(ctx, splats, off, flat, alpha, last, v_d, cum, V, W, H),
}
ms = {k: [] for k in CASES}
ops.blend_fwd(ctx, splats, off, flat, V, W, H)   # the contribution masks both backward kernels walk
for rep in range(-5, REPS):   # negative: warm-up
    for name, fn in CASES.items():
        if name.startswith("blend_fwd"):
            continue   # (timed below: it rewrites the masks, which is harmless, but keep the pairs adjacent)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if name == "blend_depth_fwd":   # its partner first, alternating
            f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f0.record(); CASES["blend_fwd (3 channels)"](); f1.record()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if rep >= 0:
            ms[name].append(e0.elapsed_time(e1))
            if name == "blend_depth_fwd":
                ms["blend_fwd (3 channels)"].append(f0.elapsed_time(f1))
print(f"SYNTH-1M, {V} x {W}x{H}, {flat.numel()} records, {REPS} launches each (median / min ms)")
for name in CASES:
    print(f"  {name:55s} {statistics.median(ms[name]):8.3f} {min(ms[name]):8.3f}")
