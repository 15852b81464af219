"""Inputs and the reference shared by the tests of the per-pixel loss weights (csrc/loss.hip: the WGT instantiations,
st3r_loss_l1_ssim_weighted, st3r_ctx_set_loss_weight): weight-map builders and a float64 torch-autograd reference of

    n1 = max(sum_p w, 1)                    n2 = max(sum_{p in I} w, 1)          I: rows 5 .. H-6, columns 5 .. W-6
    L1 = sum_p w sum_ch |gt - r| / (3 n1)   S = sum_{p in I} w sum_ch (1 - ssim(p, ch)) / (3 n2)
    loss = w_l1 L1 + w_ssim S

written afresh here: the window of loss_adam_cases.window(), a valid convolution, clamped variances as in
oracle/gs_torch_ref.ssim_mean.  The weight multiplies the SSIM MAP at the window's centre; the windows are unweighted."""
import functools

import numpy as np
import torch

import loss_adam_cases as lac

C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- weight builders: (H, W, seed) -> [H,W] float32 ----
def w_uniform(H, W, seed):
    """uniform random in [0, 2]"""
    return np.random.default_rng(seed).uniform(0.0, 2.0, (H, W)).astype(np.float32)


def w_holes(H, W, seed):
    """0/1: two rectangular holes (one reaches the border) and 30 % random holes"""
    rng = np.random.default_rng(seed)
    w = (rng.uniform(0, 1, (H, W)) >= 0.3).astype(np.float32)
    w[H // 4:H // 4 + max(1, H // 3), W // 5:W // 5 + max(1, W // 3)] = 0.0
    w[H - max(1, H // 5):, W // 2:] = 0.0
    return w


def w_ones(H, W, seed):
    return np.ones((H, W), np.float32)


def w_zero(H, W, seed):
    return np.zeros((H, W), np.float32)


def w_border_pixel(H, W, seed):
    """a single non-zero pixel, in the border (outside I): row 2 (or the last row of a flat image), last column"""
    w = np.zeros((H, W), np.float32)
    w[min(2, H - 1), W - 1] = 1.5
    return w


def w_interior_only(H, W, seed):
    """non-zero (uniform in (0.25, 1.25)) only inside I; all zero when the image has no interior"""
    w = np.zeros((H, W), np.float32)
    if H > 10 and W > 10:
        w[5:H - 5, 5:W - 5] = np.random.default_rng(seed).uniform(0.25, 1.25, (H - 10, W - 10)).astype(np.float32)
    return w


# name -> builder of one view's map; "zero_view" is resolved per view by weights_for
WEIGHTS = {"uniform": w_uniform, "holes": w_holes, "ones": w_ones, "border_pixel": w_border_pixel,
           "interior_only": w_interior_only, "zero_view": None}


def weights_for(name, Cn, H, W, seed):
    """[Cn,H,W] float32 of builder `name`, every view its own draw.  "zero_view": all zero in the LAST view (the only one
    of a single view), uniform in the others."""
    if name == "zero_view":
        maps = [w_uniform(H, W, seed + c) for c in range(Cn - 1)] + [w_zero(H, W, seed)]
    else:
        maps = [WEIGHTS[name](H, W, seed + c) for c in range(Cn)]
    return np.stack(maps)


# ---- the reference ----
def _conv_valid(a, g):
    """separable 11 x 11 convolution of a [H,W,3] over the interior -> [H-10,W-10,3]"""
    H, W = a.shape[0], a.shape[1]
    tmp = sum(g[k] * a[:, k:k + W - 10] for k in range(11))
    return sum(g[k] * tmp[k:k + H - 10] for k in range(11))


def ssim_map(X, Y):
    """the SSIM map of X against Y ([H,W,3] torch, H, W > 10) over the interior: float32 window weights, torchmetrics
    constants, variances clamped at 0"""
    g = torch.tensor(lac.window(), dtype=X.dtype)
    mx, my = _conv_valid(X, g), _conv_valid(Y, g)
    sxx = torch.clamp(_conv_valid(X * X, g) - mx * mx, min=0)
    syy = torch.clamp(_conv_valid(Y * Y, g) - my * my, min=0)
    sxy = _conv_valid(X * Y, g) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def weighted_loss_grad(x, y, w, dtype=torch.float64, w_l1=lac.W_L1, w_ssim=lac.W_SSIM):
    """One view: dict(l1 = weighted mean L1, ssim = weighted mean SSIM (sum_I w ssim / (3 n2)), loss, n1, n2, sum_i = sum_I w,
    grad = d loss / d x as float64 numpy) by autograd in `dtype` on the CPU."""
    H, W = x.shape[:2]
    X = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    Y = torch.tensor(np.asarray(y), dtype=dtype)
    Wt = torch.tensor(np.asarray(w), dtype=dtype)
    n1 = torch.clamp(Wt.sum(), min=1.0)
    l1 = (Wt[..., None] * (Y - X).abs()).sum() / (3 * n1)
    if H > 10 and W > 10:
        wi = Wt[5:H - 5, 5:W - 5]
        sum_i = wi.sum()
        n2 = torch.clamp(sum_i, min=1.0)
        ws = (wi[..., None] * ssim_map(X, Y)).sum() / (3 * n2)
        s = sum_i / n2 - ws          # sum_I w sum_ch (1 - ssim) / (3 n2)
    else:
        sum_i = torch.zeros((), dtype=dtype); n2 = torch.ones((), dtype=dtype)
        ws = torch.zeros((), dtype=dtype); s = torch.zeros((), dtype=dtype)
    loss = w_l1 * l1 + w_ssim * s
    loss.backward()
    grad = X.grad if X.grad is not None else torch.zeros_like(X)
    return dict(l1=float(l1.detach()), ssim=float(ws.detach()), loss=float(loss.detach()), n1=float(n1), n2=float(n2),
                sum_i=float(sum_i), grad=grad.numpy().astype(np.float64))


def grad_errors(v, ref):
    """lac.grad_errors, with (0, 0) for an all-zero reference that is met exactly (a view without weight)"""
    ref = np.asarray(ref, np.float64)
    if not np.abs(ref).max() > 0:
        return (0.0, 0.0) if not np.abs(np.asarray(v, np.float64)).max() > 0 else (np.inf, np.inf)
    return lac.grad_errors(v, ref)


@functools.lru_cache(maxsize=None)
def float32_reference_error(content, H, W, img_seed, builder, Cn, c, w_seed):
    """grad_errors of this reference evaluated in float32 against itself in float64, on the images
    lac.BUILDERS[content](H, W, img_seed) under view c of weights_for(builder, Cn, H, W, w_seed): the yardstick of a float32
    kernel where cancellation dominates."""
    x, y = lac.BUILDERS[content](H, W, img_seed)
    w = weights_for(builder, Cn, H, W, w_seed)[c]
    g32 = weighted_loss_grad(x, y, w, torch.float32)["grad"]
    g64 = weighted_loss_grad(x, y, w, torch.float64)["grad"]
    return grad_errors(g32, g64)
