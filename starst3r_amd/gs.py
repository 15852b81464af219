"""3D Gaussian Splatting refinement -- drop-in for the reference's `starster.gs`
(starster/gs.py:14-166; docs/api.rst "3DGS refinement"): same function names, arguments, defaults,
return values and `scene.*` attributes, with every per-iteration operation running in
libst3r_hip.so (no gsplat, no torchmetrics, no autograd graph in the training loop).

Reference quirks that are reproduced on purpose: scales/opacities are rendered RAW
(gs.py:79-80) while the regularisers treat them as log / logit (gs.py:132,134); sh0 is allocated and
given an optimiser but never rendered (gs.py:25,29 vs :81); colours are initialised as 1 - colour in every
SH row (gs.py:29-31); both regularisers are added once per view (gs.py:150-152); `step` restarts at 0 on
every run_3dgs_optim call (gs.py:143) while the Adam step counters persist.

Not in the reference: scene.activations = True replaces the first quirk by the canonical 3DGS parameterisation -- the
scales tensor holds log-scales, the opacities tensor logits, and renderer, regularisers and MCMC refinement read them the
same way (csrc/gs_activation.hip; activate_3dgs converts a raw scene).  Off by default.
"""
__all__ = (
    "activate_3dgs",
    "init_3dgs",
    "render_3dgs",
    "render_3dgs_original",
    "run_3dgs_optim",
    "train",
)

import contextlib
import types

import numpy as np
import torch

from . import dist as _dist
from . import ops
from . import _lib as _lib_mod

GAUSSIAN_KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")
ADAM_BLOCKS = (("means", 3), ("quats", 4), ("scales", 3), ("opacities", 1), ("shN", 12))  # block layout of [23N]


class FusedAdam:
    """Stands where the reference keeps one torch.optim.Adam per tensor (gs.py:37): exposes the slice of the
    fused optimiser state (exp_avg, exp_avg_sq, step) that belongs to one parameter."""

    def __init__(self, owner, key):
        self._owner, self.key = owner, key

    @property
    def param_groups(self):  # always the live parameter (growth replaces the tensors)
        o = self._owner
        return [dict(params=[o.scene.gaussians[self.key]], lr=o.lr, betas=o.betas, eps=o.eps)]

    @property
    def state(self):
        o = self._owner
        if self.key == "sh0":  # never receives a gradient in the reference (grad is None): no state
            return {}
        sl = o.block_slice(self.key)
        return {self.param_groups[0]["params"][0]: dict(step=o.step, exp_avg=o.m[sl], exp_avg_sq=o.v[sl])}

    def step(self):
        raise RuntimeError("the fused optimiser is stepped by run_3dgs_optim (st3r_adam_step), not per tensor")

    def zero_grad(self, set_to_none=True):
        pass


class _OptimState:
    def __init__(self, scene, lr):
        N = scene.gaussians["means"].shape[0]
        dev = scene.gaussians["means"].device
        self.scene, self.lr, self.betas, self.eps, self.step, self.N = scene, lr, (0.9, 0.999), 1e-8, 0, N
        self.m = torch.zeros(23 * N, device=dev); self.v = torch.zeros(23 * N, device=dev)
        self.grads = torch.empty(23 * N, device=dev)

    def grow(self, n_total):
        """Zero-extend the moments to n_total Gaussians (block layout: every block moves)."""
        N = self.N
        m = torch.zeros(23 * n_total, device=self.m.device); v = torch.zeros_like(m)
        off = 0
        for _, w in ADAM_BLOCKS:
            m[off * n_total:off * n_total + w * N].copy_(self.m[off * N:(off + w) * N])
            v[off * n_total:off * n_total + w * N].copy_(self.v[off * N:(off + w) * N])
            off += w
        self.m, self.v, self.N = m, v, n_total
        self.grads = torch.empty(23 * n_total, device=m.device)
        if getattr(self, "sh_m", None) is not None:   # scene.sh_degree 2 or 3: the high SH rows' block grows with it
            pad = torch.zeros((n_total - self.sh_m.shape[0], self.sh_m.shape[1]), device=m.device)
            self.sh_m, self.sh_v = torch.cat([self.sh_m, pad]), torch.cat([self.sh_v, pad])
            self.sh_grad = torch.zeros_like(self.sh_m)

    def block_slice(self, key):
        off = 0
        for k, w in ADAM_BLOCKS:
            if k == key:
                return slice(off * self.N, (off + w) * self.N)
            off += w
        raise KeyError(key)


class SSIM:
    """Callable stand-in for torchmetrics StructuralSimilarityIndexMeasure(data_range=1) (gs.py:39):
    `ssim(preds, target)` with (B,3,H,W) tensors returns the mean SSIM, computed by st3r_loss_l1_ssim."""

    def __init__(self, device):
        self.device = torch.device(device)

    def to(self, device):
        self.device = torch.device(device)
        return self

    def __call__(self, preds, target):
        ctx = ops.get_context(self.device)
        x = preds.permute(0, 2, 3, 1).contiguous().float(); y = target.permute(0, 2, 3, 1).contiguous().float()
        sums, _ = ops.loss_l1_ssim(ctx, x, y, 1.0, 0.0, want_grad=False)
        H, W = x.shape[1], x.shape[2]
        return (sums[:, 1] / ((H - 10) * (W - 10) * 3)).mean().float()


class MCMCStrategy:
    """Stands where the reference constructs gsplat.MCMCStrategy() (gs.py:43-45) with its default
    hyper-parameters; the three refinement operations run in libst3r_hip.so (csrc/mcmc.hip):

      step_post_backward(step, lr): inside the refine window (500 < step < 25000, every 100 steps) dead
      Gaussians are relocated onto alive ones and the set grows by 5 % up to cap_max; position noise is
      injected on every call.  Opacities/scales are read as logits/logs here while the renderer uses the
      same tensors raw -- the reference's behaviour; with scene.activations = True the renderer
      reads them as logits/logs too.

    Random draws come from a counter-based generator keyed by state["seed"] and a call counter, not from
    torch's global generator: view-sharded replicas take identical decisions with no communication."""
    cap_max = 1_000_000; noise_lr = 5e5; refine_start_iter = 500; refine_stop_iter = 25_000
    refine_every = 100; min_opacity = 0.005

    def check_sanity(self, params, optimizers):
        for k in ("means", "scales", "quats", "opacities"):
            assert k in params and k in optimizers, f"{k} is required"

    def initialize_state(self, seed=0):
        return {"binoms": None, "seed": int(seed), "calls": 0, "n_relocated": 0, "n_added": 0}

    def step_pre_backward(self, params, optimizers, state, step, info):
        return None

    def is_refine_step(self, step):
        return self.refine_start_iter < step < self.refine_stop_iter and step % self.refine_every == 0

    def refine(self, params, optimizers, state, step, call):
        """relocate dead Gaussians + grow by 5 % (needs every Gaussian: the full, replicated tensors)."""
        owner = optimizers["means"]._owner
        ctx = ops.get_context(params["means"].device)
        seed = state.get("seed", 0)
        P = {k: params[k].data for k in GAUSSIAN_KEYS}
        state["n_relocated"] = ops.mcmc_relocate(ctx, P, owner.m, owner.v, self.min_opacity, seed, call)
        N = P["means"].shape[0]
        if getattr(owner, "sh_m", None) is not None and owner.sh_m.shape[0] == N:
            # scene.sh_degree 2 or 3: the moments of the high SH rows restart where the relocation restarted the others --
            # on the Gaussians it drew as sources (the draw counts the context keeps, st3r_ctx_peek 7)
            src = ops.peek(ctx, 7, N, torch.int32) > 0
            owner.sh_m[src] = 0.0
            owner.sh_v[src] = 0.0
        n_new = max(0, min(self.cap_max, int(1.05 * N)) - N)
        if n_new > 0:
            grown = {}
            for k in GAUSSIAN_KEYS:
                t = torch.empty((N + n_new,) + tuple(P[k].shape[1:]), dtype=P[k].dtype, device=P[k].device)
                t[:N].copy_(P[k])
                grown[k] = t
            ops.mcmc_add(ctx, grown, N, n_new, self.min_opacity, seed, call)
            for k in GAUSSIAN_KEYS:  # new leaf tensors, as gsplat re-creates the nn.Parameters
                params[k] = torch.nn.Parameter(grown[k], requires_grad=True)
            owner.grow(N + n_new)
        state["n_added"] = n_new

    def step_post_backward(self, params, optimizers, state, step, info, lr):
        ctx = ops.get_context(params["means"].device)
        seed, call = state.get("seed", 0), state.get("calls", 0)
        state["calls"] = call + 1
        with torch.no_grad():
            if self.is_refine_step(step):
                self.refine(params, optimizers, state, step, call)
            P = {k: params[k].data for k in ("means", "quats", "scales", "opacities")}
            ops.mcmc_noise(ctx, P, lr * self.noise_lr, seed, call)


def _activations(scene):
    """scene.activations (absent: False): do the scales hold log-scales and the opacities logits; ValueError unless a bool"""
    on = getattr(scene, "activations", False)
    if not isinstance(on, bool):
        raise ValueError(f"scene.activations is True or False, got {on!r}")
    return on


def _sh_degree(scene):
    """scene.sh_degree (absent or None: nothing about any call changes): the SH degree the scene's colours are evaluated at,
    an int 0..3; ValueError for a bool or anything else"""
    d = getattr(scene, "sh_degree", None)
    if d is None:
        return None
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) <= 3:
        raise ValueError(f"scene.sh_degree is None or an int 0..3, got {d!r}")
    return int(d)


@contextlib.contextmanager
def _sh_setting(ctx, degree, active=None, v_sh_high=None):
    """the ctx evaluates SH at `degree` (ops.set_sh_degree) inside the block and at what it had before behind it; None:
    nothing is set"""
    if degree is None:
        yield
        return
    prev = ops.set_sh_degree(ctx, degree, active, v_sh_high)
    try:
        yield
    finally:
        ops.set_sh_degree(ctx, *prev)


def init_3dgs(scene, init_scale=3e-3, lr=1e-3):
    """Initialize 3DGS splats and optims from Mast3r dense points (reference gs.py:14-45).

    With scene.activations = True (not in the reference) the scales are log(init_scale) and the opacities
    logit(scene.init_opacity) -- init_opacity a setting of the scene, default 0.1 as in gsplat's trainer; an init_scale
    <= 0 or an init_opacity outside (0, 1) raises ValueError before anything is allocated.  Everything else is as without.
    With scene.sh_degree set to an int (not in the reference) sh0 and row 0 of shN are (colour - 0.5) / C0 and rows 1..23 are
    zero -- the canonical initialisation; the reference fills all 24 rows with 1 - colour, which at degree 3 would start
    training from strong spurious view dependence.  With the setting absent or None the tensors are the reference's."""
    scale_0, opacity_0 = init_scale, 1.0
    if _activations(scene):
        p = getattr(scene, "init_opacity", 0.1)
        if isinstance(p, bool) or not isinstance(p, (int, float, np.floating, np.integer)) or not 0.0 < float(p) < 1.0:
            raise ValueError(f"scene.init_opacity is a float in (0, 1), got {p!r}")
        if isinstance(init_scale, bool) or not isinstance(init_scale, (int, float, np.floating, np.integer)) or \
                not (float(init_scale) > 0.0 and np.isfinite(float(init_scale))):
            raise ValueError(f"scene.activations = True stores log(init_scale): init_scale must be a finite float > 0, "
                             f"got {init_scale!r}")
        scale_0 = float(np.log(np.float64(init_scale)))
        opacity_0 = float(np.log(np.float64(p)) - np.log1p(-np.float64(p)))
    pts = scene.dense_pts_flat
    colors = scene.dense_cols_flat
    n = pts.shape[0]
    g = {
        "means": pts.clone().float(),
        "scales": torch.full_like(pts, scale_0, dtype=torch.float32),
        "quats": torch.zeros(n, 4),
        "opacities": torch.full((n,), opacity_0),
        "sh0": torch.zeros(n, 1, 3),
        "shN": torch.zeros(n, 24, 3),
    }
    g["quats"][:, 0] = 1.0
    if _sh_degree(scene) is None:
        inv = (1 - colors).float()
        g["sh0"][:, 0] = inv
        g["shN"][:] = inv[:, None, :]
    else:   # canonical: the DC term alone carries the colour, C0 k0 + 0.5 = colour; no spurious view dependence
        dc = (colors.float() - 0.5) / 0.2820947917738781
        g["sh0"][:, 0] = dc
        g["shN"][:, 0] = dc
    scene.gaussians = {k: torch.nn.Parameter(v.to(scene.device).contiguous(), requires_grad=True) for k, v in g.items()}
    scene._gs_optim = _OptimState(scene, lr)
    scene.optimizers = {k: FusedAdam(scene._gs_optim, k) for k in scene.gaussians}
    scene.ssim = SSIM(scene.device)
    scene.strategy = MCMCStrategy()
    scene.strategy.check_sanity(scene.gaussians, scene.optimizers)
    scene.strategy_state = scene.strategy.initialize_state()
    scene._gt_dev = None


def activate_3dgs(scene, eps=1e-4):
    """Convert a raw scene (scales and opacities rendered as they are) to the canonical parameterisation in place:
    scales <- log(max(|s|, 1e-30)) (the covariance only ever saw s^2), opacities <- logit(clamp(o, eps, 1 - eps)), both
    formed in float64; scene.activations = True.  The Adam moments of the two blocks are zeroed -- the parameter space
    changed -- while the other blocks' moments and the step counter stay.  The render of the converted scene is the raw
    scene's wherever its opacities lay in [eps, 1 - eps].  ValueError on a scene that is activated already."""
    if _activations(scene):
        raise ValueError("scene.activations is True already: the scales are log-scales and the opacities logits")
    if not 0.0 < float(eps) < 0.5:
        raise ValueError(f"eps is a float in (0, 0.5), got {eps!r}")
    g, st = scene.gaussians, scene._gs_optim
    with torch.no_grad():
        s = g["scales"].data.double().abs().clamp(min=1e-30)
        g["scales"].data.copy_(torch.log(s))
        o = g["opacities"].data.double().clamp(float(eps), 1.0 - float(eps))
        g["opacities"].data.copy_(torch.log(o) - torch.log1p(-o))
        for key in ("scales", "opacities"):
            st.m[st.block_slice(key)] = 0.0
            st.v[st.block_slice(key)] = 0.0
    scene.activations = True


RENDER_MODES = ("RGB", "D", "ED", "RGB+D", "RGB+ED")   # gsplat.rasterization's render_mode


class _Activate(torch.autograd.Function):
    """S = exp(scales), O = sigmoid(opacities) in front of _Rasterize (st3r_param_activate / st3r_param_activate_bwd):
    differentiable into the log-scales and the logits; the backward reads the stored S and O."""

    @staticmethod
    def forward(fctx, scales, opacities, ctx):
        S, O, _ = ops.param_activate(ctx, scales.detach().contiguous(), opacities.detach().contiguous())
        fctx.save_for_backward(S, O)
        fctx.ctx = ctx
        return S, O

    @staticmethod
    def backward(fctx, v_S, v_O):
        S, O = fctx.saved_tensors
        v_s, v_o = ops.param_activate_bwd(fctx.ctx, S, O, v_S.contiguous().float(), v_O.contiguous().float())
        return v_s, v_o, None


class _Rasterize(torch.autograd.Function):
    """Differentiable wrapper so user code can still back-propagate through render_3dgs: into the Gaussians, when
    w2c requires a gradient into the camera poses, and with want_Ks into the intrinsics (st3r_gs_intrinsics_bwd).
    want_depth: returns (rgb, alpha, depth) -- the depth map of the same
    render (st3r_gs_blend_depth_fwd) -- and back-propagates from any of them; without it (rgb, alpha), and no depth
    kernel runs, forward or backward.  The per-pair gradients of the colour and of the depth backward are summed and go
    through project_sh_bwd / viewmat_bwd once; the depth column (z of the record) is added by st3r_gs_depth_bwd."""

    @staticmethod
    def forward(fctx, means, quats, scales, opacities, shN, w2c, Ks, width, height, ctx, want_depth, want_Ks=False,
                sh_degree=None):
        with _sh_setting(ctx, sh_degree):
            rgb, alpha, info = ops.rasterization(ctx, means, quats, scales, opacities, shN, w2c, Ks, width, height)
        fctx.save_for_backward(means, quats, scales, opacities, shN, w2c, Ks, alpha)
        fctx.info, fctx.ctx, fctx.wh, fctx.want_Ks, fctx.sh_degree = info, ctx, (width, height), want_Ks, sh_degree
        if not want_depth:
            return rgb, alpha
        fctx.set_materialize_grads(False)   # an output the loss does not use costs no backward kernel
        depth = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                                    info["_last_ids"], w2c.shape[0], width, height)
        return rgb, alpha, depth

    @staticmethod
    def backward(fctx, v_rgb, v_alpha, v_depth=None):
        means, quats, scales, opacities, shN, w2c, Ks, alpha = fctx.saved_tensors
        info, ctx, (W, H) = fctx.info, fctx.ctx, fctx.wh
        Cn, N = w2c.shape[0], means.shape[0]
        lists = (info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"])
        # the backward kernels consume the contribution masks the forward left in the ctx: re-run the blend forward so
        # that they belong to THIS rasterization even if other renders happened in between
        ops.blend_fwd(ctx, *lists, Cn, W, H)
        v_splats = None
        if v_rgb is not None or v_alpha is not None:
            v_rgb = torch.zeros((Cn, H, W, 3), device=alpha.device) if v_rgb is None else v_rgb.contiguous().float()
            v_splats = ops.blend_bwd(ctx, *lists, alpha, info["_last_ids"], v_rgb,
                                     None if v_alpha is None else v_alpha.contiguous().float(), info["_cum_tiles"], Cn, W, H)
        if v_depth is not None:
            v_d = ops.blend_depth_bwd(ctx, *lists, alpha, info["_last_ids"], v_depth.contiguous().float(),
                                      info["_cum_tiles"], Cn, W, H)
            v_splats = v_d if v_splats is None else v_splats.add_(v_d)   # (disjoint: colour floats 6-8, depth float 9)
        if v_splats is None:
            v_splats = torch.zeros_like(info["_splats"])
        # scene.sh_degree: the two kernels that evaluate SH run at the degree of the forward; the rows 4.. of v_shN
        deg, v_hi = fctx.sh_degree, None
        if deg is not None and deg >= 2:
            v_hi = torch.empty((N, 3 * (ops.sh_rows(deg) - 4)), dtype=torch.float32, device=means.device)
        # camera poses: only when asked for (gsplat's v_viewmats); intrinsics: only with scene.intrinsics_grad
        # (gsplat returns none) -- the depth column of v_splats does not depend on K
        v_w2c = v_Ks = None
        with _sh_setting(ctx, deg, deg, v_hi):
            grads = ops.project_sh_bwd(ctx, means, quats, scales, opacities, shN, w2c, Ks, info["_campos"], W, H,
                                       info["_splats"], v_splats)
            if fctx.needs_input_grad[5]:
                v_w2c = ops.viewmat_bwd(ctx, means, quats, scales, shN, w2c, Ks, info["_campos"], W, H, info["_splats"],
                                        v_splats)
        if fctx.want_Ks and fctx.needs_input_grad[6]:
            v4 = ops.intrinsics_bwd(ctx, means, quats, scales, w2c, Ks, W, H, info["_splats"], v_splats)
            v_Ks = torch.zeros_like(Ks)
            v_Ks[:, 0, 0] = v4[:, 0]; v_Ks[:, 1, 1] = v4[:, 1]; v_Ks[:, 0, 2] = v4[:, 2]; v_Ks[:, 1, 2] = v4[:, 3]
        if v_depth is not None:
            ops.depth_bwd(ctx, means, w2c, info["_splats"], v_splats, grads, v_w2c)
        G = ops.split_grads(grads, N)
        v_sh = torch.zeros_like(shN)
        v_sh[:, :4] = G["sh"]
        if v_hi is not None:
            v_sh[:, 4:ops.sh_rows(deg)] = v_hi.view(N, -1, 3)
        return G["means"], G["quats"], G["scales"], G["opacities"], v_sh, v_w2c, v_Ks, None, None, None, None, None, None


class _Exposure(torch.autograd.Function):
    """y = A x + t per view (st3r_exposure_fwd / st3r_exposure_bwd): differentiable into the render and the exposures."""

    @staticmethod
    def forward(fctx, rgb, exposure, ctx):
        rgb, exposure = rgb.contiguous(), exposure.contiguous()
        fctx.save_for_backward(rgb, exposure)
        fctx.ctx = ctx
        return ops.exposure_fwd(ctx, rgb, exposure)

    @staticmethod
    def backward(fctx, v_out):
        rgb, exposure = fctx.saved_tensors
        v_rgb, v_exposure = ops.exposure_bwd(fctx.ctx, rgb, exposure, v_out.contiguous().float())
        return v_rgb, v_exposure, None


class _Composite(torch.autograd.Function):
    """y = x + (1 - alpha) b per view (st3r_composite_fwd / st3r_alpha_grad): differentiable into the render, its alpha
    and the backgrounds."""

    @staticmethod
    def forward(fctx, rgb, alpha, backgrounds, ctx):
        rgb, alpha, backgrounds = rgb.contiguous(), alpha.contiguous(), backgrounds.contiguous()
        fctx.save_for_backward(alpha, backgrounds)
        fctx.ctx = ctx
        return ops.composite_fwd(ctx, rgb, alpha, backgrounds)

    @staticmethod
    def backward(fctx, v_out):
        alpha, backgrounds = fctx.saved_tensors
        v_out = v_out.contiguous().float()
        v_alpha, _, v_b = ops.alpha_grad(fctx.ctx, alpha, backgrounds, v_out, want_v_backgrounds=fctx.needs_input_grad[2])
        return v_out, v_alpha, v_b, None


def _render_backgrounds(scene, n_views, render_mode):
    """scene.render_backgrounds as the (n_views, 3) tensor of this render, or None; its checks, before anything runs"""
    B = getattr(scene, "render_backgrounds", None)
    if B is None or B is False:
        return None
    if render_mode in ("D", "ED"):
        raise ValueError(f"scene.render_backgrounds applies to the RGB channels: render_mode {render_mode!r} has none")
    if B is True:
        B = getattr(scene, "backgrounds", None)
        if B is None:
            raise ValueError("scene.render_backgrounds = True needs scene.backgrounds, one colour per image: there are none")
        B = torch.as_tensor(np.asarray(B) if not torch.is_tensor(B) else B, dtype=torch.float32)
    if not torch.is_tensor(B) or tuple(B.shape) != (n_views, 3):
        shape = tuple(B.shape) if torch.is_tensor(B) else type(B).__name__
        raise ValueError(f"scene.render_backgrounds must be None, True or a tensor of shape ({n_views}, 3), one colour per "
                         f"rendered view, got {shape}")
    return B


def _check_render_exposure(exposure, n_views, render_mode):
    """the checks of render_3dgs(exposure=...), before anything runs"""
    if render_mode in ("D", "ED"):
        raise ValueError(f"exposure applies to the RGB channels: render_mode {render_mode!r} has none")
    if not torch.is_tensor(exposure) or tuple(exposure.shape) != (n_views, 3, 4):
        shape = tuple(exposure.shape) if torch.is_tensor(exposure) else type(exposure).__name__
        raise ValueError(f"exposure must be a tensor of shape ({n_views}, 3, 4), one [A | t] per view, got {shape}")


def render_3dgs(scene, w2c: torch.Tensor, intrinsics: torch.Tensor, width: int, height: int, render_mode: str = "RGB",
                exposure=None):
    """Render the splats from a set of camera views (reference gs.py:47-88).

    Returns the tuple the reference gets from gsplat.rasterization: (render_img (N,H,W,3),
    render_alpha (N,H,W,1), info).  render_mode follows gsplat: "D" (accumulated depth sum_i w_i z_i) and "ED"
    (expected depth D / clamp(alpha, min=1e-10)) return render_img (N,H,W,1); "RGB+D" and "RGB+ED" return (N,H,W,4)
    with the depth last.  Every mode back-propagates into the Gaussians and, when it requires a gradient, into w2c.
    exposure (not in the reference): a (N,3,4) tensor, one affine colour transform [A | t] per view, applied to the RGB
    channels of render_img (y = A x + t); differentiable into the Gaussians, w2c and exposure.
    scene.render_backgrounds (gsplat.rasterization's `backgrounds`, which the reference does not pass on; a setting of the
    scene like intrinsics_grad, for the same reason; absent or None: off): a (N,3) tensor, one colour per rendered view,
    under the RGB channels of render_img (y = x + (1 - alpha) b), before exposure -- scene first, then camera; True stands
    for scene.backgrounds, the colours run_3dgs_optim trains against (N = len(scene.imgs), as in render_3dgs_original;
    ValueError when there are none).  The depth channel of "RGB+D" / "RGB+ED" gets no background (gsplat pads it with 0),
    "D" / "ED" raise ValueError as they do for exposure; differentiable into the Gaussians (through the colours and through
    alpha), w2c, the intrinsics (under scene.intrinsics_grad) and the tensor itself.
    scene.intrinsics_grad (not in the reference; gsplat returns no such gradient; a setting of the scene, default False,
    because the argument list above is the boundary users program against): True makes the backward pass return
    d loss / d intrinsics as well when `intrinsics` requires a gradient -- (N,3,3), non-zero at fx, fy, cx, cy -- in every
    render_mode; with False no kernel for it runs and intrinsics.grad stays None.
    scene.activations (not in the reference; a setting of the scene, default False; anything but a bool raises ValueError):
    True reads scene.gaussians["scales"] as log-scales and ["opacities"] as logits -- the render sees exp and sigmoid of
    them (st3r_param_activate) in every render_mode and with every option above, back-propagates into the logs and logits,
    and info["opacities"] holds the activated values, as in gsplat.
    scene.sh_degree (not in the reference, which evaluates degree 1 on rows 0..3 of shN; a setting of the scene; absent or
    None: exactly that; a bool or anything but an int 0..3 raises ValueError): the colours are evaluated at this degree, on
    rows 0 .. (sh_degree + 1)^2 - 1 of shN (st3r_ctx_set_sh_degree, set around the call and restored behind it), in every
    render_mode and with every option above; the backward pass fills those rows of shN.grad and takes the pose gradient
    through the same degree."""
    if render_mode not in RENDER_MODES:
        raise ValueError(f"render_mode must be one of {RENDER_MODES}, got {render_mode!r}")
    activated = _activations(scene)
    sh_degree = _sh_degree(scene)
    backgrounds = _render_backgrounds(scene, w2c.shape[0], render_mode)
    if exposure is not None:
        _check_render_exposure(exposure, w2c.shape[0], render_mode)
    g = scene.gaussians
    ctx = ops.get_context(scene.device)
    w2c = w2c.to(scene.device, torch.float32).contiguous(); Ks = intrinsics.to(scene.device, torch.float32).contiguous()
    if exposure is not None:
        exposure = exposure.to(scene.device, torch.float32)
    if backgrounds is not None:
        backgrounds = backgrounds.to(scene.device, torch.float32)
    scales, opacities = _Activate.apply(g["scales"], g["opacities"], ctx) if activated else (g["scales"], g["opacities"])
    out = _Rasterize.apply(g["means"], g["quats"], scales, opacities, g["shN"], w2c, Ks, width, height, ctx,
                           render_mode != "RGB", bool(getattr(scene, "intrinsics_grad", False)), sh_degree)
    if render_mode == "RGB":
        rgb, alpha = out
        if backgrounds is not None:
            rgb = _Composite.apply(rgb, alpha, backgrounds, ctx)
        img = rgb if exposure is None else _Exposure.apply(rgb, exposure, ctx)
    else:
        rgb, alpha, depth = out
        if render_mode.endswith("ED"):
            depth = depth / alpha.clamp(min=1e-10)
        if backgrounds is not None and render_mode.startswith("RGB"):
            rgb = _Composite.apply(rgb, alpha, backgrounds, ctx)
        if exposure is not None and render_mode.startswith("RGB"):
            rgb = _Exposure.apply(rgb, exposure, ctx)
        img = torch.cat([rgb, depth], dim=-1) if render_mode.startswith("RGB") else depth
    # the info dict of the most recent rasterization (gsplat's `meta`)
    info = {k: v for k, v in ops.last_info().items() if not k.startswith("_")}
    return img, alpha, info


def render_3dgs_original(scene, width: int, height: int, render_mode: str = "RGB", exposure=False):
    """Render from camera views of original scene (reference gs.py:90-95).  exposure=True (not in the reference): through
    the trained scene.exposures (run_3dgs_optim(exposure_lr=...)), i.e. as the photographs were taken.  With
    scene.render_backgrounds = True the render lies over scene.backgrounds (see render_3dgs)."""
    if exposure:
        E = getattr(scene, "exposures", None)
        if E is None:
            raise ValueError("exposure=True needs trained exposures: scene.exposures does not exist "
                             "(run_3dgs_optim(exposure_lr=...) creates it)")
        return scene.render_3dgs(scene.w2c, scene.intrinsics, width, height, render_mode=render_mode, exposure=E)
    if render_mode == "RGB":
        return scene.render_3dgs(scene.w2c, scene.intrinsics, width, height)
    return scene.render_3dgs(scene.w2c, scene.intrinsics, width, height, render_mode=render_mode)


def _gt_on_device(scene, views):
    """GT images are uploaded once and cached (the reference re-uploads every view every iteration, gs.py:151)."""
    key = (tuple(views), len(scene.imgs))
    if getattr(scene, "_gt_dev", None) is None or scene._gt_dev[0] != key:
        imgs = [torch.as_tensor(np.asarray(scene.imgs[i]), dtype=torch.float32) for i in views]
        scene._gt_dev = (key, torch.stack(imgs).to(scene.device).contiguous())
        scene._gt_mom = None
    return scene._gt_dev[1]


def _gt_moments(scene, ctx, gt):
    """SSIM's windowed moments of the ground truth, conv(gt) and conv(gt^2): the reference recomputes them every iteration
    (torchmetrics, gs.py:129) although the images never change; here once per uploaded image set."""
    if getattr(scene, "_gt_mom", None) is None or scene._gt_mom[0] is not gt:
        scene._gt_mom = (gt, ops.gt_moments(ctx, gt))
    return scene._gt_mom[1]


def _depth_prior_on_device(scene, views, conf_thres, height, width):
    """scene.depth_maps and the 0/1 weights (depth_confs > conf_thres; all ones without confidences) of `views`, uploaded
    once and cached like the ground truth (keyed by the tensors and their versions; a numpy map edited in place is not
    noticed: assign a new one).  Raises ValueError on missing or mis-shaped maps."""
    maps, confs = getattr(scene, "depth_maps", None) or [], getattr(scene, "depth_confs", None) or []
    if len(maps) != len(scene.imgs):
        raise ValueError(f"depth_fac != 0 needs one depth map per image in scene.depth_maps: {len(maps)} maps, "
                         f"{len(scene.imgs)} images")
    if confs and len(confs) != len(scene.imgs):
        raise ValueError(f"scene.depth_confs holds {len(confs)} maps for {len(scene.imgs)} images")
    for name, lst in (("depth_maps", maps), ("depth_confs", confs)):
        for i in (views if lst else ()):
            if tuple(lst[i].shape) != (height, width):
                raise ValueError(f"scene.{name}[{i}] has shape {tuple(lst[i].shape)}, its image ({height}, {width})")
    stamp = lambda t: (id(t), getattr(t, "_version", None))   # a map edited in place is uploaded again
    key = (tuple(views), tuple(stamp(maps[i]) for i in views), tuple(stamp(confs[i]) for i in views) if confs else None,
           float(conf_thres))
    if getattr(scene, "_depth_dev", None) is None or scene._depth_dev[0] != key:
        z = torch.stack([torch.as_tensor(maps[i], dtype=torch.float32) for i in views]).to(scene.device).contiguous()
        if confs:
            w = torch.stack([torch.as_tensor(confs[i], dtype=torch.float32) for i in views]).to(scene.device)
            w = (w > conf_thres).to(torch.float32).contiguous()
        else:
            w = torch.ones_like(z)
        scene._depth_dev = (key, z, w, [maps[i] for i in views], [confs[i] for i in views] if confs else None)
    return scene._depth_dev[1], scene._depth_dev[2]


def _view_indices(n_views, freeze, option):
    """sorted view indices of the option `freeze` (negative ones count from the end); ValueError outside [-n_views, n_views)"""
    out = set()
    for i in freeze:
        if isinstance(i, bool) or int(i) != i or not -n_views <= int(i) < n_views:
            raise ValueError(f"{option} holds {i!r}: not the index of one of the {n_views} views")
        out.add(int(i) % n_views)
    return sorted(out)


def _exposure_frozen(n_views, exposure_freeze):
    """_view_indices of exposure_freeze"""
    return _view_indices(n_views, exposure_freeze, "exposure_freeze")


def _on(value, schedule=False):
    """is the option this rate or factor belongs to switched on: not 0.0 or, for a rate, a callable schedule"""
    return (schedule and callable(value)) or float(value) != 0.0


def _rate_at(rate, step):
    """value at `step` of a rate given as a float or as a callable step -> float"""
    return float(rate(step)) if callable(rate) else float(rate)


def _freeze_mask(n, frozen, device):
    """[n] ones, zeros at the sorted indices `frozen`: the mask of the per-view Adam steps"""
    mask = torch.ones(n, device=device)
    if frozen:
        mask[frozen] = 0.0
    return mask


def _per_view_moments(st, name, n, device):
    """st.<name>_m, st.<name>_v ([n] zeros) and st.<name>_step (0): made on first use or when n changed, else kept"""
    m = getattr(st, name + "_m", None)
    if m is None or m.numel() != n:
        setattr(st, name + "_m", torch.zeros(n, device=device))
        setattr(st, name + "_v", torch.zeros(n, device=device))
        setattr(st, name + "_step", 0)


def _frozen_rows_kept(new, old, frozen):
    """`new` (the caller's own tensor) on old's device and in its dtype, the rows `frozen` taken from `old` bit for bit"""
    new = new.to(device=old.device, dtype=old.dtype)
    if frozen:
        new[frozen] = old.detach()[frozen]
    return new


def _single_replica_only(option, scene, enable_pruning):
    """the refusal of a per-view option (named as the user spelled it) under torch.distributed or the sharded layout"""
    if _dist.rank_world()[1] > 1 or _sharded_layout(scene, 1, enable_pruning):
        raise NotImplementedError(f"{option} != 0 is supported in a single process with replicated Gaussians only "
                                  "(not under torch.distributed, not with ST3R_MULTI_GPU=gaussian-sharded)")


class _PerViewOption:
    """One per-view option of run_3dgs_optim: everything the call does for it.  run_3dgs_optim builds the options that are
    on (when_on) and walks them at each of the hooks below; an option overrides those it needs.  `c` is what the call
    works on: scene, ctx, st (scene._gs_optim), views, width, height, gt, and the w2c and Ks of the views, which an option
    that trains them replaces by a private copy."""
    spelled = None     # the rate or factor that switches it on, as the user spells it
    schedule = True    # may that value be a callable step -> float
    counter = None     # name of its Adam step counter on scene._gs_optim: moves wherever st.step moves

    @classmethod
    def when_on(cls, scene, enable_pruning, value, *args):
        """the option's object, refused or checked before anything runs -- None when `value` leaves it off"""
        if not _on(value, schedule=cls.schedule):
            return None
        _single_replica_only(cls.spelled, scene, enable_pruning)
        return cls(scene, value, *args)

    def set_up(self, c):
        """once c.views, c.w2c, c.Ks and c.gt exist: private copies, moments, masks, buffers"""

    def register(self, c):
        """with the ctx, for the duration of the call"""

    def clear(self, c):
        """what register registered"""

    def behind_step(self, c, step):
        """its own launch behind iteration `step`'s training step, on the same stream"""

    def finish(self, c):
        """whatever ends the loop: what the scene gets back"""


class _DepthPrior(_PerViewOption):
    """depth_fac: the views' depth maps and 0/1 weights, registered with the ctx for the fused step's depth term"""
    spelled, schedule = "depth_fac", False

    def __init__(self, scene, depth_fac, conf_thres):
        self.fac, self.conf_thres = float(depth_fac), conf_thres

    def set_up(self, c):
        self.prior, self.weights = _depth_prior_on_device(c.scene, c.views, self.conf_thres, c.height, c.width)

    def register(self, c):
        ops.set_depth_prior(c.ctx, c.gt, self.prior, self.weights, self.fac)

    def clear(self, c):
        ops.set_depth_prior(c.ctx, None, None, None)


class _Poses(_PerViewOption):
    """pose_lr: the step itself moves the cameras (ops.train_step_poses, with step_args); scene.c2w follows at the end"""
    spelled, counter = "pose_lr", "pose_step"

    def __init__(self, scene, pose_lr, pose_freeze):
        self.rate, self.freeze = pose_lr, pose_freeze

    def set_up(self, c):
        # a private copy: the tensor Scene.w2c caches is never trained (c.w2c may be a view of it)
        c.w2c = c.w2c.clone()
        n_cam = c.w2c.shape[0]
        _per_view_moments(c.st, "pose", 6 * n_cam, c.w2c.device)   # (new when the views changed)
        # pose_freeze is NOT validated like the other two freeze lists (_view_indices): its indices are taken modulo the
        # number of cameras.  Kept as it is; tightening it would change behaviour.
        self.frozen = sorted({int(i) % n_cam for i in self.freeze})
        self.mask = _freeze_mask(n_cam, self.frozen, c.w2c.device)
        c.st.pose_w2c = c.w2c   # the matrices being trained (diagnostics; scene.c2w follows when the loop ends)

    def step_args(self, st, step):
        """the arguments ops.train_step_poses takes behind ops.train_step's"""
        return st.pose_m, st.pose_v, _rate_at(self.rate, step), st.pose_step, self.mask

    def finish(self, c):   # a NEW c2w tensor, so that Scene.w2c's cache refreshes itself; inverted in double
        c.scene.c2w = _frozen_rows_kept(torch.inverse(c.w2c.double()), c.scene.c2w, self.frozen)


class _Exposures(_PerViewOption):
    """exposure_lr: scene.exposures, trained in place by their own Adam behind the step, from the gradient the step
    leaves in st.exp_grad"""
    spelled, counter = "exposure_lr", "exp_step"

    def __init__(self, scene, exposure_lr, exposure_freeze):
        self.rate, self.frozen = exposure_lr, _exposure_frozen(len(scene.imgs), exposure_freeze)

    def set_up(self, c):
        scene, st, dev = c.scene, c.st, c.gt.device
        n_img = len(scene.imgs)
        E = getattr(scene, "exposures", None)
        if E is None or tuple(E.shape) != (n_img, 3, 4):   # first use, or the number of images changed
            E = torch.eye(3, 4, device=dev).repeat(n_img, 1, 1)
        if E.dtype != torch.float32 or E.device != dev or not E.is_contiguous():
            E = E.detach().to(dev, torch.float32).contiguous()
        scene.exposures = E   # trained in place
        _per_view_moments(st, "exp", 12 * n_img, dev)
        st.exp_grad = torch.zeros((n_img, 3, 4), device=dev)   # this step's d loss / d exposures (diagnostics)
        self.mask = _freeze_mask(n_img, self.frozen, dev)

    def register(self, c):
        ops.set_exposure(c.ctx, c.gt, c.scene.exposures, c.st.exp_grad)

    def clear(self, c):
        ops.set_exposure(c.ctx, None, None, None)

    def behind_step(self, c, step):   # behind the same device-side guard as the step's updates
        st = c.st
        ops.exposure_adam_step(c.ctx, c.scene.exposures, st.exp_grad, st.exp_m, st.exp_v, _rate_at(self.rate, step),
                               st.betas[0], st.betas[1], st.eps, st.exp_step, self.mask)


class _Intrinsics(_PerViewOption):
    """scene.intrinsics_lr: a private copy of the views' intrinsics, trained in place by its own Adam behind the step, which
    wrote st.k_grad at the intrinsics it started with; scene.intrinsics follows at the end"""
    spelled, counter = "scene.intrinsics_lr", "k_step"

    def __init__(self, scene, intrinsics_lr):
        self.rate = intrinsics_lr
        self.frozen = _view_indices(len(scene.imgs), getattr(scene, "intrinsics_freeze", ()), "scene.intrinsics_freeze")
        self.tie_focal = bool(getattr(scene, "intrinsics_tie_focal", True))
        self.opt_pp = bool(getattr(scene, "intrinsics_opt_pp", False))

    def set_up(self, c):
        c.Ks = c.Ks.clone()   # a private copy, trained in place
        n_k = c.Ks.shape[0]
        _per_view_moments(c.st, "k", 4 * n_k, c.Ks.device)   # (new when the views changed)
        c.st.k_grad = torch.zeros((n_k, 4), device=c.Ks.device)   # this step's d loss / d (fx, fy, cx, cy) (diagnostics)
        self.mask = _freeze_mask(n_k, self.frozen, c.Ks.device)

    def register(self, c):
        ops.set_intrinsics_grad(c.ctx, c.gt, c.st.k_grad)

    def clear(self, c):
        ops.set_intrinsics_grad(c.ctx, None, None)

    def behind_step(self, c, step):
        st = c.st
        ops.intrinsics_adam_step(c.ctx, c.Ks, st.k_grad, st.k_m, st.k_v, _rate_at(self.rate, step), st.betas[0],
                                 st.betas[1], st.eps, st.k_step, self.mask, c.width, c.height, self.tie_focal, self.opt_pp)

    def finish(self, c):   # a NEW intrinsics tensor (the private copy), device and dtype as before
        c.scene.intrinsics = _frozen_rows_kept(c.Ks, c.scene.intrinsics, self.frozen)


def _loss_masks_key(masks, height, width):
    """what the cached upload of scene.loss_masks is keyed by: the entries' identities and versions (a numpy map edited in
    place is not noticed: assign a new one) and the image size"""
    return (tuple(None if m is None else (id(m), getattr(m, "_version", None)) for m in masks), height, width)


def _check_loss_masks(scene, masks, height, width):
    """ValueError unless scene.loss_masks is one entry per image, each None or an [H,W] map of finite values >= 0.  The
    values of maps that are already uploaded (same key) are not scanned again."""
    if isinstance(masks, (np.ndarray, torch.Tensor)) or not hasattr(masks, "__len__"):
        raise ValueError("scene.loss_masks is a list with one entry per image (None or an [H,W] map), "
                         f"got {type(masks).__name__}")
    if len(masks) != len(scene.imgs):
        raise ValueError(f"scene.loss_masks holds {len(masks)} entries for {len(scene.imgs)} images")
    for i, m in enumerate(masks):
        if m is not None and tuple(getattr(m, "shape", ())) != (height, width):
            raise ValueError(f"scene.loss_masks[{i}] has shape {tuple(getattr(m, 'shape', ()))}, its image "
                             f"({height}, {width})")
    cached = getattr(scene, "_loss_mask_dev", None)
    if cached is not None and cached[0] == _loss_masks_key(masks, height, width):
        return
    for i, m in enumerate(masks):
        if m is None:
            continue
        t = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m))
        if t.dtype == torch.bool:
            continue
        if t.is_complex() or not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError(f"scene.loss_masks[{i}] holds negative or non-finite entries: weights are finite and >= 0")


def _loss_masks_on_device(scene, masks, views, height, width):
    """the weight maps of `views` ([views,H,W] float32, contiguous; None entries are all ones), uploaded once and cached
    like the depth prior's maps"""
    key = _loss_masks_key(masks, height, width)
    cached = getattr(scene, "_loss_mask_dev", None)
    if cached is None or cached[0] != key or cached[1] != tuple(views):
        def on_device(m):
            if m is None:
                return torch.ones((height, width), dtype=torch.float32, device=scene.device)
            m = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m))
            return m.detach().to(scene.device, torch.float32)
        w = torch.stack([on_device(masks[i]) for i in views]).contiguous()
        scene._loss_mask_dev = (key, tuple(views), w, list(masks))   # (the entries are kept: their ids stay theirs)
    return scene._loss_mask_dev[2]


class _LossMasks(_PerViewOption):
    """scene.loss_masks: per-pixel weights of the photometric loss, registered with the ctx for the fused step's weighted
    L1 + SSIM"""
    spelled, schedule = "scene.loss_masks", False

    @classmethod
    def when_on(cls, scene, enable_pruning, masks):
        """switched on by a list, not by a rate: off when absent, None, or every entry None"""
        if masks is None:
            return None
        height, width = scene.imgs[0].shape[:2]
        _check_loss_masks(scene, masks, height, width)
        if all(m is None for m in masks):
            return None
        _single_replica_only(cls.spelled, scene, enable_pruning)
        return cls(scene, masks)

    def __init__(self, scene, masks):
        self.masks = masks

    def set_up(self, c):
        self.weights = _loss_masks_on_device(c.scene, self.masks, c.views, c.height, c.width)

    def register(self, c):
        ops.set_loss_weight(c.ctx, c.gt, self.weights)

    def clear(self, c):
        ops.set_loss_weight(c.ctx, None, None)


def _as_tensor(a):
    """a tensor or whatever numpy makes an array of, as a (detached) tensor"""
    return a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


class _Backgrounds(_PerViewOption):
    """scene.backgrounds: one fixed colour per image under its render, registered with the ctx for the fused step's composite"""
    spelled, schedule = "scene.backgrounds", False

    @classmethod
    def when_on(cls, scene, enable_pruning, backgrounds):
        """switched on by the colours themselves: off when absent or None"""
        if backgrounds is None:
            return None
        try:
            b = _as_tensor(backgrounds)
        except Exception:
            b = None
        n = len(scene.imgs)
        if b is None or b.dtype == torch.bool or b.is_complex() or tuple(b.shape) != (n, 3):
            shape = type(backgrounds).__name__ if b is None else f"{b.dtype} {tuple(b.shape)}"
            raise ValueError(f"scene.backgrounds is one colour per image, a numeric array or tensor of shape ({n}, 3), got {shape}")
        if not bool(torch.isfinite(b.double()).all()):
            raise ValueError("scene.backgrounds holds non-finite entries")
        _single_replica_only(cls.spelled, scene, enable_pruning)
        return cls(scene, backgrounds, b)

    def __init__(self, scene, backgrounds, as_tensor):
        self.given, self.tensor = backgrounds, as_tensor

    def set_up(self, c):   # uploaded once and cached like the loss masks (identity and version of what the scene holds)
        key = (id(self.given), getattr(self.given, "_version", None), tuple(c.views))
        cached = getattr(c.scene, "_backgrounds_dev", None)
        if cached is None or cached[0] != key:
            colors = self.tensor.to(c.scene.device, torch.float32)[list(c.views)].contiguous()
            c.scene._backgrounds_dev = (key, colors, self.given)   # (the object is kept: its id stays its own)
        self.colors = c.scene._backgrounds_dev[1]

    def register(self, c):
        ops.set_background(c.ctx, c.gt, self.colors)

    def clear(self, c):
        ops.set_background(c.ctx, None, None)


def _alpha_maps_key(masks, weights, height, width):
    """what the cached upload of scene.alpha_masks / alpha_weights is keyed by (as _loss_masks_key)"""
    return (_loss_masks_key(masks, height, width), None if weights is None else _loss_masks_key(weights, height, width))


def _check_alpha_maps(scene, name, maps, height, width, upper):
    """ValueError unless scene.<name> is one entry per image, each None or an [H,W] map, bool or numeric, of finite values
    in [0, upper] (upper None: >= 0)"""
    if isinstance(maps, (np.ndarray, torch.Tensor)) or not hasattr(maps, "__len__"):
        raise ValueError(f"scene.{name} is a list with one entry per image (None or an [H,W] map), got {type(maps).__name__}")
    if len(maps) != len(scene.imgs):
        raise ValueError(f"scene.{name} holds {len(maps)} entries for {len(scene.imgs)} images")
    for i, m in enumerate(maps):
        if m is not None and tuple(getattr(m, "shape", ())) != (height, width):
            raise ValueError(f"scene.{name}[{i}] has shape {tuple(getattr(m, 'shape', ()))}, its image ({height}, {width})")
    for i, m in enumerate(maps):
        if m is None:
            continue
        t = _as_tensor(m)
        if t.dtype == torch.bool:
            continue
        bad = t.is_complex() or not bool(torch.isfinite(t).all()) or bool((t < 0).any()) or \
            (upper is not None and bool((t > upper).any()))
        if bad:
            allowed = "finite and >= 0" if upper is None else f"finite and in [0, {upper}]"
            raise ValueError(f"scene.{name}[{i}] holds entries out of range: the values are {allowed}")


class _AlphaMasks(_PerViewOption):
    """scene.alpha_fac with scene.alpha_masks / scene.alpha_weights: per-view targets of the render's accumulated opacity,
    registered with the ctx for the fused step's alpha term"""
    spelled, schedule = "scene.alpha_fac", False

    @classmethod
    def when_on(cls, scene, enable_pruning, alpha_fac, masks, weights):
        """the maps are checked whenever they are there; off when alpha_fac == 0 or every mask is None"""
        if isinstance(alpha_fac, bool) or not isinstance(alpha_fac, (int, float, np.floating, np.integer)) or \
                not np.isfinite(float(alpha_fac)):
            raise ValueError(f"scene.alpha_fac is a plain finite float, got {alpha_fac!r}")
        height, width = scene.imgs[0].shape[:2]
        cached = getattr(scene, "_alpha_maps_dev", None)
        scanned = cached is not None and masks is not None and cached[0] == _alpha_maps_key(masks, weights, height, width)
        if masks is not None and not scanned:   # (the values of maps that are already uploaded are not scanned again)
            _check_alpha_maps(scene, "alpha_masks", masks, height, width, 1)
        if weights is not None and not scanned:
            _check_alpha_maps(scene, "alpha_weights", weights, height, width, None)
        if float(alpha_fac) == 0.0:
            return None
        if masks is None:
            raise ValueError("scene.alpha_fac != 0 needs one target per image in scene.alpha_masks: there are none")
        if all(m is None for m in masks):
            return None
        _single_replica_only(cls.spelled, scene, enable_pruning)
        return cls(scene, float(alpha_fac), masks, weights)

    def __init__(self, scene, alpha_fac, masks, weights):
        self.fac, self.masks, self.weight_maps = alpha_fac, masks, weights

    def set_up(self, c):   # uploaded once and cached like the loss masks
        scene, H, W = c.scene, c.height, c.width
        key = _alpha_maps_key(self.masks, self.weight_maps, H, W)
        cached = getattr(scene, "_alpha_maps_dev", None)
        if cached is None or cached[0] != key or cached[1] != tuple(c.views):
            def on_device(m, fill):
                if m is None:
                    return torch.full((H, W), fill, dtype=torch.float32, device=scene.device)
                return _as_tensor(m).to(scene.device, torch.float32)
            target = torch.stack([on_device(self.masks[i], 0.0) for i in c.views]).contiguous()
            # a view without a target is not supervised: weight 0 whatever alpha_weights holds for it
            weight = torch.stack([on_device(None if self.masks[i] is None or self.weight_maps is None else self.weight_maps[i],
                                            0.0 if self.masks[i] is None else 1.0) for i in c.views]).contiguous()
            scene._alpha_maps_dev = (key, tuple(c.views), target, weight, list(self.masks),
                                     None if self.weight_maps is None else list(self.weight_maps))
        self.target, self.weights = scene._alpha_maps_dev[2], scene._alpha_maps_dev[3]

    def register(self, c):
        ops.set_alpha_target(c.ctx, c.gt, self.target, self.weights, self.fac)

    def clear(self, c):
        ops.set_alpha_target(c.ctx, None, None, None)


class _Activations(_PerViewOption):
    """scene.activations: the ctx reads the scales as log-scales and the opacities as logits for the duration of the call.
    No per-view data, but the same life cycle: refused like the per-view options, set where they register, cleared where
    they clear."""
    spelled, schedule = "scene.activations", False

    @classmethod
    def when_on(cls, scene, enable_pruning):
        if not _activations(scene):
            return None
        _single_replica_only(cls.spelled, scene, enable_pruning)
        return cls()

    def register(self, c):
        ops.set_activation(c.ctx, True)

    def clear(self, c):
        ops.set_activation(c.ctx, False)


def _sh_active_degree(t, interval, degree):
    """the degree the step with 1-based Adam counter t evaluates: one more band every `interval` steps (gsplat's trainer),
    the full degree from the first step with interval 0"""
    return degree if interval <= 0 else min((t - 1) // interval, degree)


class _ShDegree(_PerViewOption):
    """scene.sh_degree: the ctx evaluates SH at the scene's degree -- at the schedule's active degree, step by step -- for
    the duration of the call, and the rows 4.. of shN are trained by an Adam step of their own behind the training step.
    Its gradient buffer and moments live on scene._gs_optim (sh_grad, sh_m, sh_v [N, 3 (rows - 4)], sh_step)."""
    spelled, schedule, counter = "scene.sh_degree", False, "sh_step"

    @classmethod
    def when_on(cls, scene, enable_pruning):
        degree = _sh_degree(scene)
        if degree is None:
            return None
        interval = getattr(scene, "sh_degree_interval", 0)
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or interval < 0:
            raise ValueError(f"scene.sh_degree_interval is an int >= 0, got {interval!r}")
        rate = getattr(scene, "sh_high_lr", None)
        if rate is not None and (isinstance(rate, bool) or not isinstance(rate, (int, float, np.floating, np.integer))
                                 or not float(rate) >= 0.0):
            raise ValueError(f"scene.sh_high_lr is None or a float >= 0, got {rate!r}")
        _single_replica_only(cls.spelled, scene, enable_pruning)
        if enable_pruning and degree >= 2 and type(getattr(scene, "strategy", None)) is not MCMCStrategy:
            raise NotImplementedError("scene.sh_degree >= 2 together with enable_pruning needs the project's own "
                                      "MCMCStrategy: another strategy object does not carry the moments of the SH rows 4..")
        return cls(degree, int(interval), rate)

    def __init__(self, degree, interval, rate):
        self.degree, self.interval, self.rate = degree, interval, rate
        self.rows = max(ops.sh_rows(degree), 4)   # rows of the compact SH copy the loop trains

    def set_up(self, c):
        st, n = c.st, c.scene.gaussians["means"].shape[0]
        if not hasattr(st, "sh_step"):
            st.sh_step = 0
        if self.degree < 2:
            return
        width = 3 * (self.rows - 4)
        m = getattr(st, "sh_m", None)
        if m is None or m.shape[1] != width:          # first use, or another degree: a new parameter block
            st.sh_m = torch.zeros((0, width), device=c.scene.device); st.sh_v = torch.zeros_like(st.sh_m)
            st.sh_step = 0
        if st.sh_m.shape[0] != n:                     # the set grew: the new Gaussians start from zero moments
            grow = lambda t: torch.cat([t[:n], torch.zeros((max(n - t.shape[0], 0), width), device=t.device)])
            st.sh_m, st.sh_v = grow(st.sh_m), grow(st.sh_v)
        st.sh_grad = torch.zeros((n, width), device=c.scene.device)

    def before_step(self, c, sh):
        """the setting of this step: its active degree by the Gaussians' Adam counter"""
        self.active = _sh_active_degree(c.st.step, self.interval, self.degree)
        self.sh = sh
        ops.set_sh_degree(c.ctx, self.degree, self.active, c.st.sh_grad if self.degree >= 2 else None)

    def clear(self, c):
        ops.set_sh_degree(c.ctx, *ops.SH_DEFAULT)

    def behind_step(self, c, step):
        if self.degree >= 2:
            st = c.st
            ops.sh_high_adam_step(c.ctx, self.sh, self.degree, st.sh_grad, st.sh_m, st.sh_v,
                                  st.lr if self.rate is None else float(self.rate), st.betas[0], st.betas[1], st.eps,
                                  st.sh_step)


def _iterations(iters, verbose):
    """range(iters), with a progress bar when verbose"""
    if verbose:
        from tqdm import trange
        return trange(iters)
    return range(iters)


@contextlib.contextmanager
def _registered(c, options=()):
    """What is registered with c.ctx belongs to the call: the moments of the ground truth c.gt, then the options' buffers --
    cleared in that order whatever ends the block, a failing registration included."""
    try:
        ops.set_gt_moments(c.ctx, c.gt, _gt_moments(c.scene, c.ctx, c.gt))
        for o in options:
            o.register(c)
        yield
    finally:
        ops.set_gt_moments(c.ctx, None, None)
        for o in options:
            o.clear(c)


def _losses_list(losses, iters):
    """the per-iteration losses summed over the ranks: one device->host copy for the whole call (reference: .item() per step)"""
    _dist.all_reduce_sum(losses)
    return losses[:iters].cpu().tolist()


def run_3dgs_optim(
        scene,
        iters: int,
        enable_pruning: bool = False,
        loss_ssim_fac=0.2,
        loss_opacity_fac=0.01,
        loss_scale_fac=0.01,
        verbose: bool = False,
        pose_lr=0.0,
        pose_freeze=(),
        depth_fac=0.0,
        depth_conf_thres=1.5,
        exposure_lr=0.0,
        exposure_freeze=(),
    ) -> list:
    """Run 3DGS optimization and pruning (optional) for a number of iterations (reference gs.py:97-166).

    Returns the list of per-iteration losses (floats).  Under torch.distributed (one process per GPU, RCCL)
    the views are sharded over the ranks, the [23N] gradient buffer is sum-all-reduced every iteration and
    every rank applies the identical fused Adam update; the returned losses are the sums over all views.

    pose_lr (not in the reference; a float or a callable step -> float): when not 0.0 the cameras are optimised jointly
    with the Gaussians, inside the same fused step (Adam on a left se(3) perturbation of every world-to-camera matrix,
    ops.train_step_poses); the views listed in pose_freeze stay fixed.  A callable receives the iteration index of THIS
    call (0 .. iters-1), like the returned losses -- a second call restarts the schedule, while the pose moments and
    their step counter (bias correction) continue.  The loop trains a private copy of the poses; when
    it ends scene.c2w is REPLACED by a new tensor, the inverse of the refined matrices (frozen views keep their rows bit
    for bit).  The pose moments and step counter persist on scene._gs_optim like the Gaussians'.  Single process,
    Gaussians replicated only.

    depth_fac (not in the reference): when not 0.0 the loss of every view gains a depth term inside the same fused step,
    depth_fac * sum_p w |ED - Z| / max(sum_p w, 1): ED the expected depth of the render (render_mode "ED"), Z the view's
    map in scene.depth_maps (Scene.add_images keeps the alignment's; they are in the gauge of the poses, so nothing is
    fitted) and w = 1 where scene.depth_confs exceeds depth_conf_thres, else 0 (all ones when depth_confs is empty).  Works
    together with pose_lr and enable_pruning; single process, Gaussians replicated only.

    exposure_lr (not in the reference; a float or a callable step -> float as pose_lr): when not 0.0 every view gets an
    affine colour transform y = A x + t between its render and the loss, inside the same fused step, trained by its own
    Adam (the Gaussians' betas and eps) from the identity: photographs taken with auto-exposure and auto-white-balance
    disagree photometrically, and without it the Gaussians explain that with view-dependent colour and floaters.  The
    transforms live in scene.exposures [len(scene.imgs),3,4] (float32, on the device; created as identities on first use or
    when the number of images changed) and are trained in place; their moments and step counter persist on
    scene._gs_optim (exp_m, exp_v, exp_step).  The views in exposure_freeze keep their exposure bit for bit: they fix the
    gauge between colours and exposures.  render_3dgs_original(exposure=True) renders through them.  Works together with
    pose_lr, depth_fac and enable_pruning; single process, Gaussians replicated only.  With exposure_lr == 0 nothing about
    the call changes and scene.exposures is not created.

    scene.intrinsics_lr, scene.intrinsics_freeze, scene.intrinsics_tie_focal, scene.intrinsics_opt_pp (not in the reference;
    settings of the scene, defaults 0.0, (), True, False, because the argument list above is the boundary users program
    against and stays as it is).  intrinsics_lr is a float or a callable step -> float as pose_lr: when not 0.0 the views'
    intrinsics are refined inside the same fused step -- the focal the alignment estimated is off by a few per cent for
    few views, and no pose update removes that.  Adam (the Gaussians' betas and eps) on (log fx, log fy, cx / W, cy / H) of
    every view, so one rate serves every image size.  intrinsics_tie_focal (default): one focal scalar per view, fx / fy
    keeps its value; intrinsics_opt_pp: the principal point is trained too (default: it stays).  The views in
    intrinsics_freeze keep their row bit for bit.  The loop trains a private float32 copy; when it ends scene.intrinsics
    is REPLACED by a new tensor of its old dtype and device.  Moments and step counter persist on scene._gs_optim (k_m,
    k_v, k_step).  Focal length and camera distance are nearly degenerate for a single view: the intended use is together
    with pose_lr and with at least one frozen view, so that the other views' geometry decides between the two.  Works
    together with pose_lr, depth_fac, exposure_lr and enable_pruning; single process, Gaussians replicated only.  With
    intrinsics_lr == 0 nothing about the call changes and scene.intrinsics is not touched.

    scene.loss_masks (not in the reference; a setting of the scene like intrinsics_lr, default absent or None): a list with
    one entry per image, each None (all ones) or an [H,W] array or tensor, bool or numeric, finite and >= 0 -- the weight of
    every pixel in the photometric loss of its view: 0 drops the pixel (a passer-by, the sky, a watermark), 1 is the plain
    loss, anything else is allowed, so a confidence can be used directly.  Per view, with I the SSIM interior,
    loss = (1 - ssim_fac) sum_p w |gt - r| / (3 max(sum_p w, 1)) + ssim_fac sum_{p in I} w (1 - ssim) / (3 max(sum_I w, 1)).
    The weight multiplies the SSIM map at the centre of the 11 x 11 window; the windows themselves stay unweighted, so a
    pixel within 5 px (Chebyshev distance) of a weighted pixel still enters that pixel's window: grow a mask by 5 px to keep
    something out entirely.  A view whose weights are all zero contributes nothing.  The regularisers and the depth term
    (which keeps its own weights) are unchanged; the returned losses are the weighted ones.  Wrong count, wrong shape,
    negative or non-finite entries raise ValueError before anything runs.  The maps are uploaded once and cached (keyed by
    the entries' identities and versions: assign a new array instead of editing one in place).  Works together with
    pose_lr, depth_fac, exposure_lr, scene.intrinsics_lr and enable_pruning; single process, Gaussians replicated only.
    With loss_masks absent, None, or every entry None nothing about the call changes and nothing is registered.

    scene.backgrounds (not in the reference, which renders on black; a setting of the scene like loss_masks, default absent
    or None): an array or tensor [len(scene.imgs),3], finite -- the colour under every view's render inside the same fused
    step, y = x + (1 - alpha) b before the exposure (scene first, then camera): photographs of an object on a white backdrop,
    or a masked-out object composited on white, can then be trained against without Gaussians that paint the backdrop.  The
    colours are fixed, not trained; with scene.render_backgrounds = True the render calls lay them under their image.

    scene.alpha_fac, scene.alpha_masks, scene.alpha_weights (not in the reference; settings of the scene, defaults 0.0, absent,
    absent).  alpha_fac is a plain float: when not 0.0 the loss of every view gains a silhouette term inside the same fused
    step, alpha_fac * sum_p w |alpha - M| / max(sum_p w, 1), alpha the accumulated opacity of the render.  alpha_masks is a
    list with one entry per image, each None (that view is not supervised: weight 0) or an [H,W] map M in [0,1], bool or
    numeric; alpha_weights, optional, has the same layout: None entries are all ones, values are finite and >= 0, and a 0
    marks the "don't know" pixels of a trimap.  Together with loss_masks this lets an object mask do its job in the dropped
    pixels: the photometric loss ignores them, the alpha term pushes alpha to 0 outside the mask and to 1 inside it.
    alpha_fac != 0 without alpha_masks raises ValueError, as depth_fac does without depth maps; with alpha_fac == 0, or every
    mask None, the option is off.  The returned losses include the alpha term.

    For both: wrong count, wrong shape, values out of range or non-finite raise ValueError before anything runs; the uploads
    are cached and keyed like the loss masks'; they work together with pose_lr, depth_fac, exposure_lr, scene.intrinsics_lr,
    scene.loss_masks and enable_pruning; single process, Gaussians replicated only.  With both off nothing about the call
    changes and nothing is registered.

    scene.activations (not in the reference; a setting of the scene, default False; anything but a bool raises ValueError):
    True trains log-scales and logits -- the fused step renders exp(scales) and sigmoid(opacities), the regularisers are the
    reference's, loss_opacity_fac * mean(sigmoid(opacities)) and loss_scale_fac * mean(exp(scales)) once per view, now
    functions of what is rendered, and the MCMC refinement of enable_pruning reads the tensors the same way as the renderer.
    Adam, the moments and their layout do not change.  init_3dgs under the setting, or activate_3dgs on a raw scene, produce
    such tensors.  Works together with every option above and enable_pruning; single process, Gaussians replicated only.
    With the setting off nothing about the call changes.
    scene.sh_degree (not in the reference, which trains degree 1 on rows 0..3 of shN; a setting of the scene; absent or
    None: exactly that, and nothing is set on the context; a bool or anything but an int 0..3 raises ValueError): the fused
    step evaluates the colours at this degree, the compact SH copy holds (sh_degree + 1)^2 rows (at least 4), and the rows
    4.. are trained by an Adam step of their own behind every training step (st3r_sh_high_adam_step, guarded on the device
    like the Gaussians': the capacity-overflow repeat needs nothing new) at scene.sh_high_lr (None: the Gaussians' rate).
    scene.sh_degree_interval (default 0: the full degree from the first step): n > 0 evaluates, at the step with 1-based
    Adam counter t, the degree min((t - 1) // n, sh_degree) -- gsplat's trainer schedule.  The high rows' gradient and
    moments persist on scene._gs_optim (sh_grad, sh_m, sh_v, sh_step) from call to call.  Works together with every option
    above and with enable_pruning under the project's own MCMCStrategy -- relocation and growth copy whole shN rows, a
    refinement step zeroes the rows of sh_m / sh_v of the Gaussians the relocation drew as sources, and sh_grad, sh_m and
    sh_v grow with zeros when the set grows; another strategy object together with sh_degree >= 2 raises
    NotImplementedError --; single process, Gaussians replicated only.  init_3dgs under the setting starts from the
    canonical DC-only colours.
    """
    activations = _Activations.when_on(scene, enable_pruning)   # (its check comes first)
    sh_degree = _ShDegree.when_on(scene, enable_pruning)
    masks = _LossMasks.when_on(scene, enable_pruning, getattr(scene, "loss_masks", None))   # (its checks come first)
    backgrounds = _Backgrounds.when_on(scene, enable_pruning, getattr(scene, "backgrounds", None))
    alphas = _AlphaMasks.when_on(scene, enable_pruning, getattr(scene, "alpha_fac", 0.0), getattr(scene, "alpha_masks", None),
                                 getattr(scene, "alpha_weights", None))
    depth = _DepthPrior.when_on(scene, enable_pruning, depth_fac, depth_conf_thres)
    poses = _Poses.when_on(scene, enable_pruning, pose_lr, pose_freeze)
    exposures = _Exposures.when_on(scene, enable_pruning, exposure_lr, exposure_freeze)
    intrinsics = _Intrinsics.when_on(scene, enable_pruning, getattr(scene, "intrinsics_lr", 0.0))
    # in this order at every hook: checks (above), set-up, registration, clearing, behind the step, finish
    options = [o for o in (depth, poses, exposures, intrinsics, masks, backgrounds, alphas, activations, sh_degree)
               if o is not None]
    counters = [o.counter for o in options if o.counter]
    height, width = scene.imgs[0].shape[:2]
    ctx = ops.get_context(scene.device)
    st = scene._gs_optim
    g = scene.gaussians
    rank, world = _dist.rank_world()
    if _sharded_layout(scene, world, enable_pruning):
        return _run_3dgs_optim_sharded(scene, iters, loss_ssim_fac, loss_opacity_fac, loss_scale_fac, verbose,
                                       enable_pruning)
    views = _dist.shard_views(len(scene.imgs), rank, world)
    w2c = scene.w2c.to(scene.device, torch.float32)[views].contiguous()
    Ks = scene.intrinsics.to(scene.device, torch.float32)[views].contiguous()
    campos = ops.camera_positions(w2c)
    gt = _gt_on_device(scene, views)
    losses = torch.zeros(max(iters, 1), device=scene.device)
    fused = world == 1 or getattr(ctx, "native_comm", False)
    c = types.SimpleNamespace(scene=scene, ctx=ctx, st=st, views=views, width=width, height=height, gt=gt, w2c=w2c, Ks=Ks)
    for o in options:
        o.set_up(c)
    w2c, Ks = c.w2c, c.Ks   # (the private copies of the options that train them)
    restore_exchange = None
    if enable_pruning and fused and world > 1 and ops.get_exchange(ctx) in ("rs_ag", "direct"):
        # reduce-scatter exchange (through RCCL or through the peers' exported buffers): a rank maintains the Adam moments of its piece of the buffer only; growing the set
        # moves the piece boundaries, so a refinement run uses the plain all-reduce (replicated moments) for its duration:
        # the pieces are all-gathered first so that every rank holds the same, complete moments
        ops.allgather_pieces(ctx, st.m); ops.allgather_pieces(ctx, st.v)
        restore_exchange = ops.set_exchange(ctx, "allreduce")
    # The kernels touch SH rows 0..3 only (sh_degree = 1, gs.py:81,86).  Read in place those 48 bytes sit at a 288-byte
    # stride -- three streaming kernels (projection, its backward, Adam) then move ~2.7x the SH bytes they use --, so the loop
    # trains a COMPACT copy [N, 4, 3] (sh_stride = 12) and writes it back into rows 0..3 of `shN` when it ends, and before
    # every strategy hook that may look at the parameters (measured at 1 M Gaussians: projection 0.183 -> 0.157 ms, its
    # backward 0.223 -> 0.203, Adam 0.148 -> 0.105; tools/experiments/ab_compact_sh.sh).
    # (scene.sh_degree 2 or 3: the 9 or 16 rows in use)
    sh_rows = 4 if sh_degree is None else sh_degree.rows
    sh_c = [g["shN"].data[:, :sh_rows].contiguous()]

    def sh_write_back():
        g["shN"].data[:, :sh_rows].copy_(sh_c[0])

    def one_iteration(step):
        if sh_c[0].shape[0] != g["shN"].shape[0]:   # the set grew (a refinement step replaced the tensors)
            sh_c[0] = g["shN"].data[:, :sh_rows].contiguous()
        P = {k: g[k].data for k in ("means", "quats", "scales", "opacities")}  # growth replaces the tensors
        P["shN"] = sh_c[0]
        if sh_degree is not None:
            sh_degree.before_step(c, sh_c[0])
        # which step call: the one branch on a specific option, because that is how the C interface is shaped
        if poses is not None:   # the same single call, and the cameras move in it too (w2c and campos in place)
            ops.train_step_poses(ctx, P, w2c, Ks, campos, gt, width, height, loss_ssim_fac, loss_opacity_fac,
                                 loss_scale_fac, st.grads, st.m, st.v, st.lr, st.betas[0], st.betas[1], st.eps, st.step,
                                 losses[step:step + 1], *poses.step_args(st, step), want_stats=False)
        elif fused:   # the whole iteration is one C call (gradient all-reduce inside, over the ctx's communicator)
            # no host round trip in steady state (single rank; with a communicator the library sizes every step exactly)
            ops.train_step(ctx, P, w2c, Ks, campos, gt, width, height, loss_ssim_fac, loss_opacity_fac,
                           loss_scale_fac, st.grads, st.m, st.v, st.lr, st.betas[0], st.betas[1], st.eps, st.step,
                           losses[step:step + 1], want_stats=False)
        else:       # gradient all-reduce through the host framework's process group (torch.distributed -> RCCL); every
                    # step is sized exactly (want_stats): an overflow seen by one rank only would leave the others waiting
            ops.train_fwd_bwd(ctx, P, w2c, Ks, campos, gt, width, height, loss_ssim_fac, loss_opacity_fac,
                              loss_scale_fac, st.grads, losses[step:step + 1], want_stats=True)
            _dist.all_reduce_sum(st.grads)
            ops.adam_step(ctx, P, st.grads, st.m, st.v, st.lr, st.betas[0], st.betas[1], st.eps, st.step)
        for o in options:
            o.behind_step(c, step)

    def capacity_error(e):
        return getattr(e, "code", 0) == -3 and world == 1

    def count_step(d):   # the options' step counters move wherever the Gaussians' does
        st.step += d
        for name in counters:
            setattr(st, name, getattr(st, name) + d)

    # A peer failure (ST3R_ERR_PEER: the step before failed on some rank, nobody applied it) ABORTS the run on every rank
    # alike -- all ranks get the code from the same call --; the exchange form is restored whatever ends the loop.
    # our own strategy reads the parameters in step_post_backward only, and the SH rows on refinement steps only
    # (relocation / growth copy whole rows); any OTHER strategy object sees up-to-date rows at every hook call
    own_strategy = type(scene.strategy) is MCMCStrategy
    try:
        with _registered(c, options):
            step = 0
            for _ in _iterations(iters, verbose):
                if enable_pruning:
                    if not own_strategy:
                        sh_write_back()
                    scene.strategy.step_pre_backward(g, scene.optimizers, scene.strategy_state, step, None)
                    if not own_strategy:
                        sh_c[0] = g["shN"].data[:, :sh_rows].contiguous()
                count_step(1)
                try:
                    one_iteration(step)
                except _lib_mod.St3rError as e:
                    # ST3R_ERR_CAPACITY is reported by the call AFTER the asynchronous step that outgrew its buffers (> 25 %
                    # more tile intersections than the step before it).  That step's records past the capacity were dropped
                    # and its Adam update was skipped on the device (k_adam's guard), so no parameter update has to be
                    # undone: the lost iteration is repeated -- the context is back on the exactly sized path -- and then
                    # this one runs.  With enable_pruning the strategy hooks of the lost iteration have already run on the
                    # un-updated parameters (its position noise, and on a refinement step its relocation / growth): they are
                    # NOT run again, i.e. the noise of that one iteration is drawn before its update instead of after it.  A
                    # deviation of one step's noise (tests/test_gpu_api.py::test_run_3dgs_optim_repeats_...); overflows need
                    # > 25 % more tile intersections than the step before.  With pose_lr != 0 the cameras of the lost
                    # iteration did not move either (the pose update carries the same guard).
                    if not capacity_error(e):
                        raise
                    if step > 0:
                        count_step(-1)
                        one_iteration(step - 1)
                        count_step(1)
                    one_iteration(step)
                if enable_pruning:
                    touch = bool(scene.strategy.is_refine_step(step)) if own_strategy else True
                    if touch:
                        sh_write_back()
                    scene.strategy.step_post_backward(g, scene.optimizers, scene.strategy_state, step, None, 1e-3)
                    if touch:
                        sh_c[0] = g["shN"].data[:, :sh_rows].contiguous()
                step += 1
            if world == 1 and iters > 0:
                try:   # the last step's count is still in flight: settle it now so that an overflow cannot go unnoticed
                    ops.settle(ctx)
                except _lib_mod.St3rError as e:
                    if not capacity_error(e):
                        raise
                    one_iteration(iters - 1)   # its update was skipped on the device: repeat it
    finally:   # (behind the clearing of what was registered)
        if sh_c[0].shape[0] == g["shN"].shape[0]:
            sh_write_back()
        if restore_exchange is not None:   # (the moments stay complete on every rank: rs_ag goes on using its own piece)
            ops.set_exchange(ctx, restore_exchange)
        for o in options:
            o.finish(c)
    return _losses_list(losses, iters)


def _sharded_layout(scene, world, enable_pruning):
    """Gaussians AND views sharded (layout 2) is OPT-IN: ST3R_MULTI_GPU=gaussian-sharded (also with
    a single rank: tests).  The default under torch.distributed is the north_star partition -- views sharded,
    Gaussians replicated, one gradient all-reduce per iteration.  With enable_pruning the sharded loop re-assembles
    the full tensors for the refinement steps (every 100 iterations) and shards the grown set again."""
    import os
    if os.environ.get("ST3R_MULTI_GPU", "replicated") != "gaussian-sharded":
        return False
    return len(scene.imgs) % world == 0 and scene.gaussians["means"].shape[0] >= world


def _gather_rows(full, local, counts, width):
    """full [N * width] (rows of `width` floats, rank-ordered shards) <- every rank's local rows."""
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        if all(c == counts[0] for c in counts):
            tdist.all_gather_into_tensor(full.reshape(-1), local.reshape(-1).clone())   # local may be a view of full
        else:
            parts = _dist.all_gather_varlen(local.reshape(-1).clone())
            torch.cat([p.to(full.device) for p in parts], out=full.reshape(-1))
    else:
        full.reshape(-1).copy_(local.reshape(-1))


def _run_3dgs_optim_sharded(scene, iters, ssim_fac, opac_fac, scale_fac, verbose, enable_pruning=False):
    """run_3dgs_optim on the Gaussian-sharded layout: this rank trains rows [lo, hi) of the (replicated) parameter
    tensors in place, exchanging splat records with the other ranks; at the end the shards are all-gathered so that
    scene.gaussians and the optimiser state are complete on every rank again.

    enable_pruning: the position noise of every iteration is drawn per shard (keyed by the global row, so it equals
    the replicated draw); on a refinement step the shards are gathered, relocate / grow run on the full tensors --
    identically on every rank, like in the replicated layout -- and the grown set is sharded again (balanced, sizes
    differing by at most one).  Between refinement steps nothing is replicated."""
    if _activations(scene):   # (run_3dgs_optim has refused it already: a direct call)
        raise NotImplementedError("scene.activations != 0 is supported in a single process with replicated Gaussians only "
                                  "(the Gaussian-sharded loop projects raw scales and opacities)")
    height, width = scene.imgs[0].shape[:2]
    ctx = ops.get_context(scene.device)
    st = scene._gs_optim
    rank, world = _dist.rank_world()
    views = _dist.shard_views_contiguous(len(scene.imgs), rank, world)
    w2c_all = scene.w2c.to(scene.device, torch.float32).contiguous()
    Ks_all = scene.intrinsics.to(scene.device, torch.float32).contiguous()
    gt = _gt_on_device(scene, views)
    keys = ("means", "quats", "scales", "opacities", "shN")

    def shard():
        """trainer over this rank's rows of the current full tensors (views into them: updated in place)"""
        g = scene.gaussians
        N = g["means"].shape[0]
        counts = _dist.shard_counts(N, world)
        lo, hi = _dist.shard_gaussians(N, rank, world)
        n = hi - lo
        P = {k: g[k].data[lo:hi] for k in keys}
        tr = _dist.ShardedTrainer(ctx, P, N, w2c_all, Ks_all, gt, width, height, rank, world, lr=st.lr,
                                  ssim_fac=ssim_fac, opac_fac=opac_fac, scale_fac=scale_fac, counts=counts)
        off = 0
        for _, w in ADAM_BLOCKS:                                    # this shard's rows of the [23N] moment blocks
            tr.m[off * n:(off + w) * n].copy_(st.m[off * N + w * lo:off * N + w * hi])
            tr.v[off * n:(off + w) * n].copy_(st.v[off * N + w * lo:off * N + w * hi])
            off += w
        tr.t = st.step
        return tr, P, N, n, lo, counts

    def unshard(tr, P, N, n, counts):
        """every rank's rows back into the full tensors and moment blocks"""
        g = scene.gaussians
        st.step = tr.t
        for k in keys:
            _gather_rows(g[k].data, P[k], counts, g[k].data[0].numel())
        off = 0
        for _, w in ADAM_BLOCKS:
            _gather_rows(st.m[off * N:(off + w) * N], tr.m[off * n:(off + w) * n], counts, w)
            _gather_rows(st.v[off * N:(off + w) * N], tr.v[off * n:(off + w) * n], counts, w)
            off += w

    tr, P, N, n, lo, counts = shard()
    losses = torch.zeros(max(iters, 1), device=scene.device)
    strategy, state = scene.strategy, scene.strategy_state
    with _registered(types.SimpleNamespace(scene=scene, ctx=ctx, gt=gt)):
        for step in _iterations(iters, verbose):
            tr.step(losses[step:step + 1])
            if enable_pruning:   # MCMCStrategy.step_post_backward, shard-wise
                seed, call = state.get("seed", 0), state.get("calls", 0)
                state["calls"] = call + 1
                with torch.no_grad():
                    if strategy.is_refine_step(step):
                        unshard(tr, P, N, n, counts)
                        strategy.refine(scene.gaussians, scene.optimizers, state, step, call)
                        tr, P, N, n, lo, counts = shard()
                    ops.mcmc_noise(ctx, {k: P[k] for k in ("means", "quats", "scales", "opacities")},
                                   1e-3 * strategy.noise_lr, seed, call, row_offset=lo)
    unshard(tr, P, N, n, counts)
    return _losses_list(losses, iters)


train = run_3dgs_optim  # alias for the wording of BASELINE.json's north_star ("gs.train()")
