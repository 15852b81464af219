"""Times the fused training step with and without poses, at SYNTH-1M, 8 x 1080p:
  (i)   train_step;
  (ii)  train_step_poses (pose_lr = 0 and every camera masked: the same work every launch, the scene does not drift;
        k_pose_adam is launched but returns at its mask test, so the arithmetic and stores of the 8 cameras' updates --
        one thread each, about 300 double operations -- are NOT in the figure);
  (iii) the two launches the pose path adds, stand-alone: blend_bwd (its k_gather_vtile launch is the difference to the
        fused backward) and viewmat_bwd;
  (iv)  one joint iteration the autograd way: render_3dgs with w2c.requires_grad, L1 loss, backward, torch Adam on the
        five Gaussian tensors and on w2c.
HIP events around every call, (i) and (ii) alternating in one process, medians over REPS calls after warm-up.
    python tools/time_pose_step.py [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import starst3r_amd as st
from starst3r_amd import ops
from st3r_synth import synth

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
N, V, W, H = 1_000_000, 8, 1920, 1080
g, w2c, Ks = synth.make_scene(N, V, W, H)
dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda:0")
P = {k: dev(v) for k, v in g.items()}
P["shN"] = P["shN"][:, :4].contiguous()   # the compact SH rows run_3dgs_optim trains
vm, K = dev(w2c), dev(Ks)
campos = ops.camera_positions(vm)
ctx = ops.get_context("cuda:0")
gt, _, _ = ops.render(ctx, {k: dev(v) for k, v in synth.perturb_for_gt(g).items()}, vm, K, campos, W, H)
gt = gt.contiguous()
grads = torch.empty(23 * N, device="cuda:0"); m = torch.zeros_like(grads); v = torch.zeros_like(grads)
pm = torch.zeros(6 * V, device="cuda:0"); pv = torch.zeros_like(pm)
mask = torch.zeros(V, device="cuda:0")
loss = torch.zeros(1, device="cuda:0")
ADAM = (0.0, 0.9, 0.999, 1e-8, 1)   # lr = 0: the parameters stay where they are


def step_plain():
    ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, *ADAM, loss, want_stats=False)


def step_poses():
    ops.train_step_poses(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, *ADAM, loss, pm, pv, 0.0, 1, mask,
                         want_stats=False)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms = {"train_step": [], "train_step_poses": []}
for rep in range(-5, REPS):   # negative: warm-up
    a, b = timed(step_plain), timed(step_poses)
    if rep >= 0:
        ms["train_step"].append(a); ms["train_step_poses"].append(b)

# the stand-alone pieces
full = {k: dev(x) for k, x in g.items()}
rgb, alpha, info = ops.rasterization(ctx, full["means"], full["quats"], full["scales"], full["opacities"], full["shN"], vm, K,
                                     W, H)
lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
_, v_rgb = ops.loss_l1_ssim(ctx, rgb, gt, 0.8, 0.2)
v_splats = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_rgb, None, info["_cum_tiles"], V, W, H)
ms["blend_bwd stand-alone (k_blend_bwd + k_gather_vtile)"] = []
ms["viewmat_bwd stand-alone"] = []
for rep in range(-3, REPS):
    a = timed(lambda: ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_rgb, None, info["_cum_tiles"], V, W, H))
    b = timed(lambda: ops.viewmat_bwd(ctx, full["means"], full["quats"], full["scales"], full["shN"], vm, K,
                                      info["_campos"], W, H, info["_splats"], v_splats))
    if rep >= 0:
        ms["blend_bwd stand-alone (k_blend_bwd + k_gather_vtile)"].append(a); ms["viewmat_bwd stand-alone"].append(b)
del rgb, alpha, info, lists, v_rgb, v_splats

# the autograd way
scene = st.Scene(device="cuda:0")
scene.gaussians = {k: torch.nn.Parameter(x) for k, x in full.items()}
w = vm.clone().requires_grad_()
opt = torch.optim.Adam([scene.gaussians[k] for k in ("means", "quats", "scales", "opacities", "shN")] + [w], lr=0.0)


def step_autograd():
    rgb, _, _ = scene.render_3dgs(w, K, W, H)
    opt.zero_grad()
    (rgb - gt).abs().mean().backward()
    opt.step()


ms["render_3dgs autograd + torch Adam"] = []
for rep in range(-2, max(REPS // 3, 5)):
    a = timed(step_autograd)
    if rep >= 0:
        ms["render_3dgs autograd + torch Adam"].append(a)

print(f"SYNTH-1M, {V} x {W}x{H} (median / min / max ms)")
for name, xs in ms.items():
    print(f"  {name:55s} {statistics.median(xs):8.3f} {min(xs):8.3f} {max(xs):8.3f}   n={len(xs)}")
extra = statistics.median(ms["train_step_poses"]) - statistics.median(ms["train_step"])
print(f"  pose extra per step {extra:.3f} ms; autograd iteration / train_step_poses = "
      f"{statistics.median(ms['render_3dgs autograd + torch Adam']) / statistics.median(ms['train_step_poses']):.1f}x")
