"""Helpers shared by the per-view GPU tests (camera poses, depth prior, exposures, intrinsics, the view registration):
test_gpu_pose_grad, test_gpu_pose_train, test_gpu_exposure, test_gpu_depth_prior, test_gpu_intrinsics_grad,
test_gpu_intrinsics_train and test_gpu_view_registration import from here, not from each other.  The bars of those tests
were measured on exactly these inputs: seeds, shapes, noise levels and the order of the generator draws stay as they are."""
import math

import numpy as np
import torch

from oracle import gs_oracle as go
from st3r_synth import synth

B1, B2, EPS = 0.9, 0.999, 1e-8


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gen(seed):
    return torch.Generator(device="cuda:0").manual_seed(seed)


def rel_err_per_camera(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return [float((a[c] - b[c]).abs().max() / (b[c].abs().max() + 1e-30)) for c in range(b.shape[0])]


def _ulp_bound(ref, n_ulp=2):
    """n_ulp float32 ulps of the largest entry magnitude, per camera"""
    big = ref.reshape(ref.shape[0], -1).abs().max(dim=1).values.float().numpy()
    return n_ulp * np.spacing(big).astype(np.float64)


# the scenes of tests/test_gpu_gs.py
SCENES = {
    # name: (N, views, W, H, seed, scale_lo, scale_hi)
    "small": (400, 3, 96, 64, 7, 0.01, 0.08),
    "ragged": (1500, 2, 101, 75, 21, 0.01, 0.12),
    "medium": (20000, 4, 320, 240, 5, 0.004, 0.03),
    "one": (1, 1, 48, 32, 1, 0.05, 0.06),
    "many": (800, 9, 64, 48, 3, 0.01, 0.08),
    "wide": (2500, 3, 320, 240, 13, 0.08, 0.25),
    # the edges of a 256-wide reduction (test_gpu_intrinsics_grad): one block; one block and a lone Gaussian in a second one
    "n256": (256, 2, 64, 48, 31, 0.01, 0.08),
    "n257": (257, 2, 64, 48, 32, 0.01, 0.08),
}


def fuzz_scene(seed):
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(200, 1200)); V = int(rng.integers(1, 5))
    W = int(rng.integers(40, 200)); H = int(rng.integers(30, 150))
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=1e-3, scale_hi=0.5)
    g["means"] = rng.uniform(-3.6, 3.6, (N, 3)).astype(np.float32)
    g["opacities"] = rng.uniform(-0.3, 1.6, N).astype(np.float32)
    g["scales"] = (g["scales"] * rng.uniform(0.2, 5.0, (N, 3))).astype(np.float32)
    g["quats"] = (g["quats"] * rng.uniform(0.1, 3.0, (N, 1))).astype(np.float32)
    return g, w2c, Ks, W, H


def make(name):
    if name.startswith("fuzz"):
        return fuzz_scene(int(name[4:]))
    N, V, W, H, seed, lo, hi = SCENES[name]
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=lo, scale_hi=hi)
    return g, w2c, Ks, W, H


def run_hip(ctx, g, w2c, Ks, W, H):
    from starst3r_amd import ops
    P = {k: dev(v) for k, v in g.items()}
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], dev(w2c),
                                         dev(Ks), W, H)
    return P, rgb, alpha, info


def masked_cotangents(g, w2c, Ks, W, H, seed=3):
    """random v_rgb / v_alpha, zero on the pixels whose skip / stop decisions float32 does not determine (as
    test_gpu_gs.test_backward_vs_oracle)"""
    rgb_o, alpha_o, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"], w2c, Ks,
                                            W, H, want_margin=True)
    rng = np.random.default_rng(seed)
    v_rgb = rng.standard_normal(rgb_o.shape).astype(np.float32)
    v_alpha = rng.standard_normal(alpha_o.shape).astype(np.float32)
    und = ~(meta["margin"] > 1e-4)
    v_rgb[und] = 0.0; v_alpha[und] = 0.0
    return v_rgb, v_alpha


def _se3_exp(xi):
    """4x4 matrix_exp of the twist xi = (omega, v)"""
    o1, o2, o3, v1, v2, v3 = xi.unbind()
    z = torch.zeros_like(o1)
    hat = torch.stack([torch.stack([z, -o3, o2, v1]), torch.stack([o3, z, -o1, v2]),
                       torch.stack([-o2, o1, z, v3]), torch.stack([z, z, z, z])])
    return torch.linalg.matrix_exp(hat)


def _pose_errors(w_est, w_true):
    """rotation angle (rad) and camera-centre distance between two world-to-camera matrices"""
    R_e, R_t = w_est[:3, :3], w_true[:3, :3]
    ang = 2.0 * math.asin(min(1.0, float((R_e - R_t).norm()) / (2.0 * math.sqrt(2.0))))   # |R_e - R_t|_F = 2 sqrt2 sin(a/2)
    c_e = -R_e.T @ w_est[:3, 3]; c_t = -R_t.T @ w_true[:3, 3]
    return ang, float((c_e - c_t).norm())


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the fused-step tests
# ---------------------------------------------------------------------------------------------------------------------
def _setup(ctx, g, w2c, Ks, W, H, noise_seed=1):
    """device parameters, cameras and a noisy ground truth of the scene's own render"""
    from starst3r_amd import ops
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(ctx, P, vm, K, campos, W, H)
    gen = torch.Generator(device="cuda:0").manual_seed(noise_seed)
    gt = torch.clamp(rgb + 0.05 * torch.randn(rgb.shape, device="cuda:0", generator=gen), 0, 1).contiguous()
    return P, vm, K, campos, gt


def _medium(ctx):
    N, V, W, H = 20000, 3, 320, 240
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=5, scale_lo=0.004, scale_hi=0.03)
    return _setup(ctx, g, w2c, Ks, W, H) + (W, H)


def _synthetic_prior(ctx, P, vm, K, W, H, margin=None, seed=4):
    """the expected depth of the scene's own render, perturbed (5 % relative, 0.02 absolute), and a 0/1 weight map with
    holes: a third of the pixels at random, every pixel the render hardly reaches (alpha <= 0.05: the quotient ED amplifies
    float32 noise there) and, when given, the pixels whose blend decisions float32 does not determine
    -> (Z, weights, info of the rasterization)"""
    from starst3r_amd import ops
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    d = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                            info["_last_ids"], vm.shape[0], W, H)
    ed = (d / alpha.clamp(min=1e-10))[..., 0]
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    Z = ed * (1 + 0.05 * torch.randn(ed.shape, device="cuda:0", generator=gen)) + \
        0.02 * torch.randn(ed.shape, device="cuda:0", generator=gen)
    w = (alpha[..., 0] > 0.05) & (torch.rand(ed.shape, device="cuda:0", generator=gen) > 0.33)
    if margin is not None:
        w &= torch.tensor(margin > 1e-4, device="cuda:0").reshape(w.shape)
    return Z.contiguous(), w.float().contiguous(), info


class _Run:
    """the tensors of a training run through ops.train_step / ops.train_step_poses; with K the intrinsics are trained
    too: their private copy K, moments km / kv and the gradient buffer vK (preset to 7: the step must overwrite it)"""

    def __init__(self, P0, vm, campos, steps, K=None):
        N, Cn = P0["means"].shape[0], vm.shape[0]
        self.P = {k: v.clone() for k, v in P0.items()}
        self.vm, self.campos = vm.clone(), campos.clone()
        self.grads = torch.empty(23 * N, device="cuda:0")
        self.m = torch.zeros_like(self.grads); self.v = torch.zeros_like(self.grads)
        self.pm = torch.zeros(6 * Cn, device="cuda:0"); self.pv = torch.zeros_like(self.pm)
        self.K = None
        if K is not None:
            self.K = K.clone()
            self.km = torch.zeros(4 * Cn, device="cuda:0"); self.kv = torch.zeros_like(self.km)
            self.vK = torch.full((Cn, 4), 7.0, device="cuda:0")
        self.losses = torch.zeros(steps, device="cuda:0")
        self.vvm = torch.zeros((Cn, 4, 4), device="cuda:0")
        self.snaps = []

    def state(self):
        trained_K = [] if self.K is None else [self.K, self.km, self.kv]
        return [self.P[k] for k in sorted(self.P)] + [self.m, self.v, self.vm, self.campos, self.pm, self.pv] + trained_K + \
            [self.losses]


def _optim_scene(g_start, w2c_start, Ks, imgs):
    """a Scene on the GPU as init_3dgs leaves it, from numpy Gaussians and intrinsics and w2c as numpy or torch"""
    import starst3r_amd as st
    from starst3r_amd import gs
    scene = st.Scene(device="cuda:0")
    scene.imgs = [imgs[i] for i in range(imgs.shape[0])]
    scene.c2w = torch.inverse(torch.as_tensor(w2c_start).double()).float()   # CPU float32, as the reconstruction leaves it
    scene.intrinsics = torch.tensor(Ks)
    scene.gaussians = {k: torch.nn.Parameter(dev(v)) for k, v in g_start.items()}
    scene._gs_optim = gs._OptimState(scene, 1e-3)
    scene.optimizers = {k: gs.FusedAdam(scene._gs_optim, k) for k in scene.gaussians}
    scene.strategy = gs.MCMCStrategy()
    scene.strategy_state = scene.strategy.initialize_state()
    scene._gt_dev = None
    return scene


def _small_scene(depth=3.0):
    """-> (scene, W, H): _optim_scene of "small" with black images and, unless depth is None, constant depth maps"""
    g, w2c, Ks, W, H = make("small")
    imgs = np.zeros((w2c.shape[0], H, W, 3), np.float32)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
    if depth is not None:
        scene.depth_maps = [torch.full((H, W), depth) for _ in range(w2c.shape[0])]
    return scene, W, H
