"""Inputs and references shared by the CPU oracle tests and the GPU parity tests of the loss (csrc/loss.hip) and Adam
(csrc/adam.hip) kernels: image builders, the float32 error of the torch reference itself (the yardstick for a float32
kernel on inputs where cancellation dominates), a float64 separable convolution, and one oracle Adam step over the 23N
buffer layout."""
import functools

import numpy as np
import torch

from oracle import gs_oracle as go
from oracle import gs_torch_ref as tr

W_L1, W_SSIM = 0.8, 0.2


def noise(H, W, seed):
    """Uniform-noise render and a mildly perturbed ground truth (what test_l1_ssim_vs_oracle has always used)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1).astype(np.float32)
    return x, y


def structured(H, W, seed):
    """Render x and ground truth y [H,W,3] with the structure real training images have and noise lacks:
      - y = clip(x + N(0, 0.3), 0, 1): saturates at both ends;
      - the left third of x is exactly 0 (a render where alpha is 0);
      - the lower half of y is rounded to {0, 1} (flat saturated ground truth: conv(y^2) - conv(y)^2 cancels, the syy clamp
        acts);
      - y == x on a regular sub-grid of pixels (sign(x - y) = 0), black columns included.
    There is deliberately NO constant non-zero render: there E[x^2] - mu^2 is pure rounding noise, its sign -- which decides
    whether the clamped sigma_x^2 passes a gradient -- differs between float32 and float64, and no parity bar between a
    float32 kernel and a float64 reference means anything.  (An exactly zero render is different: 0 - 0 * 0 is 0 in every
    format, never negative, and both sides take the same branch.)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    y = np.clip(x + rng.normal(0, 0.3, x.shape), 0, 1).astype(np.float32)
    x[:, :W // 3] = 0.0
    y[H // 2:] = np.round(y[H // 2:])
    y[1::4, 2::5] = x[1::4, 2::5]
    return x, y


BUILDERS = {"noise": noise, "structured": structured}


def torch_loss_grad(x, y, dtype):
    """(mean L1, mean SSIM, d(W_L1 l1 + W_SSIM (1 - ssim)) / dx) by autograd of gs_torch_ref in `dtype` on the CPU."""
    X = torch.tensor(x, dtype=dtype, requires_grad=True); Y = torch.tensor(y, dtype=dtype)
    l1 = (Y - X).abs().mean()
    H, W = x.shape[:2]
    ss = tr.ssim_mean(Y, X) if (H > 10 and W > 10) else torch.zeros((), dtype=dtype)
    (W_L1 * l1 + W_SSIM * (1 - ss)).backward()
    return float(l1.detach()), float(ss.detach()), X.grad.numpy().astype(np.float64)


def grad_errors(v, ref):
    """(error against the tensor's maximum, element-wise error over the elements above 1e-3 of the maximum): the two
    figures test_l1_ssim_vs_oracle bounds."""
    v = np.asarray(v, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    err = np.abs(v - ref)
    big = np.abs(ref) > 1e-3 * scale
    return err.max() / scale, (err[big] / np.abs(ref[big])).max()


@functools.lru_cache(maxsize=None)
def float32_reference_error(content, H, W, seed):
    """grad_errors of the torch reference evaluated in float32 against itself in float64, on BUILDERS[content](H, W, seed)."""
    x, y = BUILDERS[content](H, W, seed)
    _, _, g32 = torch_loss_grad(x, y, torch.float32)
    _, _, g64 = torch_loss_grad(x, y, torch.float64)
    return grad_errors(g32, g64)


def window():
    g = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    return (g / g.sum()).astype(np.float32).astype(np.float64)   # float32 weights, like the kernels and torchmetrics


def conv_valid(a):
    """float64 separable 11 x 11 gaussian convolution of a [..., H, W, 3] over the interior: [..., H-10, W-10, 3]."""
    g = window()
    H, W = a.shape[-3], a.shape[-2]
    a = a.astype(np.float64)
    tmp = sum(g[k] * a[..., :, k:k + W - 10, :] for k in range(11))
    return sum(g[k] * tmp[..., k:k + H - 10, :, :] for k in range(11))


# ---- Adam ----
# grads / m / v are 23N floats in blocks: means[3N] quats[4N] scales[3N] opacities[N], then the 12 scalars of SH rows
# 0..3 of every Gaussian; SH rows 4..23 receive no gradient and are not touched
ADAM_BLOCKS = (("means", 3), ("quats", 4), ("scales", 3), ("opacities", 1))
ADAM_NAMES = ("means", "quats", "scales", "opacities", "shN")
ADAM_HP = (1e-3, 0.9, 0.999, 1e-8)   # lr, beta1, beta2, eps


def adam_block_slices(N):
    """name -> slice of the 23N buffer (the SH block under "shN")."""
    out, off = {}, 0
    for name, w in ADAM_BLOCKS + (("shN", 12),):
        out[name] = slice(off, off + w * N)
        off += w * N
    return out


def adam_oracle_step(ref, m_o, v_o, gr, step, hp=ADAM_HP):
    """One oracle Adam step, in place: ref is the dict of float32 parameter arrays (shN [N,24,3]: rows 0..3 are updated, the
    rest left alone), m_o / v_o / gr the 23N-float buffers."""
    N = ref["means"].shape[0]
    sl = adam_block_slices(N)
    for name, _ in ADAM_BLOCKS:
        p = ref[name].reshape(-1); mm = m_o[sl[name]]; vv = v_o[sl[name]]
        go.adam(p, gr[sl[name]], mm, vv, *hp, step)
        m_o[sl[name]] = mm; v_o[sl[name]] = vv
    p = np.ascontiguousarray(ref["shN"][:, :4, :]).reshape(-1)
    mm = m_o[sl["shN"]]; vv = v_o[sl["shN"]]
    go.adam(p, gr[sl["shN"]], mm, vv, *hp, step)
    m_o[sl["shN"]] = mm; v_o[sl["shN"]] = vv
    ref["shN"][:, :4, :] = p.reshape(N, 4, 3)


def wide_range_grads(rng, n):
    """Gradients over six decades, like a real step's (opacity gradients of far Gaussians next to SH of near ones)."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-5, 1, n)).astype(np.float32)
