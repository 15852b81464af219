"""Inputs and float64 references of the background / alpha-supervision kernels (csrc/gs_alpha.hip: k_composite_fwd,
k_alpha_grad), numpy only, no GPU.  Used by test_alpha_cases.py (CPU: the references against torch autograd, the inputs
really exact) and test_gpu_alpha.py (the kernels, bit for bit).

The inputs are dyadic, the method of per_view_kernel_cases.exposure_inputs / depth_inputs:

    alpha   in {0, 1/4, 1/2, 1}                       x, b, M   multiples of 1/16 in [0, 1]
    v, v_in multiples of 1/8 in [-2, 2]               w         multiples of 1/8 in [0, 2], with zeros, negatives and NaN
    M       NaN or inf wherever w does not count (w <= 0 or NaN)

so 1 - a is one of {1, 3/4, 1/2, 0}, (1 - a) b a multiple of 1/64 below 1, y = x + (1 - a) b exact in float32 fused or not;
b_j v_j a multiple of 1/128 below 2, t_bg and v_in + t_bg exact in float32 in any association; (1 - a) v_j a multiple of
1/32 below 2 and w |a - M| a multiple of 1/128 below 2, so their double sums over up to 2^40 pixels are exact in any order.
What is NOT exact, and is reproduced rounding by rounding: k = (float)((double)alpha_fac / n_c), the float32 product k w,
and the float32 sum (v_in + t_bg) + t_a -- each one rounding of a value that double holds exactly.

With more than one view the LAST view has no weight at all (n_c = 1, sums 0, t_a = 0 everywhere) and view 0 has a == M
on every weighted pixel (sign 0: sums 0 and t_a = 0 with n_c > 1); every other view has exact ties on every 7th weighted
pixel.  With one view: ties on every 7th weighted pixel."""
import numpy as np

ALPHA_FAC = 0.75
ALPHAS = np.array([0.0, 0.25, 0.5, 1.0], np.float32)


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def inputs(shape, seed=0):
    """-> dict of float32 arrays: x [C,H,W,3], alpha [C,H,W,1], b [C,3], v [C,H,W,3], M, w [C,H,W], v_in [C,H,W,1], and the
    bool maps on (w counts) and tie (a == M planted)"""
    C, H, W = shape
    rng = np.random.default_rng(1100 + seed + 13 * C + H * W)
    n = (C, H, W)
    alpha = rng.choice(ALPHAS, n, p=[0.2, 0.25, 0.25, 0.3])
    x = (rng.integers(0, 17, n + (3,)) / 16.0).astype(np.float32)
    b = (rng.integers(0, 17, (C, 3)) / 16.0).astype(np.float32)
    v = (rng.integers(-16, 17, n + (3,)) / 8.0).astype(np.float32)
    v_in = (rng.integers(-16, 17, n) / 8.0).astype(np.float32)
    M = (rng.integers(0, 17, n) / 16.0).astype(np.float32)
    w = (rng.integers(1, 17, n) / 8.0).astype(np.float32)
    u = rng.uniform(0, 1, n)
    w[u < 0.25] = 0.0
    w[(u >= 0.25) & (u < 0.28)] *= -1.0
    w[(u >= 0.28) & (u < 0.30)] = np.nan
    if C > 1:
        w[C - 1] = np.where(w[C - 1] > 0, 0.0, w[C - 1])
    on = w > 0
    tie = np.zeros(n, bool)
    for c in range(C):
        idx = np.flatnonzero(on[c])
        tie[c].reshape(-1)[idx if (C > 1 and c == 0) else idx[::7]] = True
    M[tie] = alpha[tie]
    off = ~on
    M[off] = np.where(rng.integers(0, 2, int(off.sum())) == 0, np.nan, np.inf).astype(np.float32)
    return dict(x=x, alpha=alpha[..., None].copy(), b=b, v=v, M=M, w=w, v_in=v_in[..., None].copy(), on=on, tie=tie)


def composite_reference(x, alpha, b, dtype=np.float64):
    """y = x + (1 - a) b in `dtype`: [C,H,W,3]"""
    x, alpha, b = (np.asarray(a, dtype) for a in (x, alpha, b))
    return x + (dtype(1) - alpha) * b[:, None, None, :]


def alpha_grad_reference(alpha, b=None, v=None, M=None, w=None, alpha_fac=ALPHA_FAC, v_in=None, rounded=True):
    """float64; rounded: rounded to float32 where gs_alpha.hip rounds (k, k w, the last sum), else no rounding anywhere (the
    function torch autograd differentiates).  b, v None: no background term; M, w None: no alpha term; v_in None: 0.
    -> dict: v_alpha [C,H,W,1], t_bg, t_a [C,H,W], v_b [C,3] (before its float32 rounding), sums, n_c [C], w64, terms"""
    r = _r32 if rounded else (lambda a: np.asarray(a, np.float64))
    a = np.asarray(alpha, np.float64)[..., 0]
    out = {}
    t_bg = np.zeros_like(a)
    if b is not None:
        b64, v64 = np.asarray(b, np.float64), np.asarray(v, np.float64)
        t_bg = -(b64[:, None, None, :] * v64).sum(-1)
        out["v_b"] = ((1.0 - a)[..., None] * v64).sum((1, 2))
    t_a = np.zeros_like(a)
    if M is not None:
        w32 = np.asarray(w, np.float32)
        on = w32 > 0
        w64 = np.where(on, w32, 0.0).astype(np.float64)
        n_c = np.maximum(w64.sum((1, 2)), 1.0)
        k = r(float(np.float32(alpha_fac) if rounded else alpha_fac) / n_c)[:, None, None]
        with np.errstate(invalid="ignore"):
            diff = np.where(on, a - np.where(on, np.asarray(M, np.float64), 0.0), 0.0)
        t_a = np.where(on, r(r(k * w64) * np.sign(diff)), 0.0)
        terms = w64 * np.abs(diff)
        out.update(sums=terms.sum((1, 2)), n_c=n_c, w64=w64, terms=terms, diff=diff)
    vin = np.zeros_like(a) if v_in is None else np.asarray(v_in, np.float64)[..., 0]
    out.update(t_bg=t_bg, t_a=t_a, v_alpha=r((vin + t_bg) + t_a)[..., None])
    return out


def alpha_grad_float32(alpha, b=None, v=None, M=None, w=None, alpha_fac=ALPHA_FAC, v_in=None):
    """the kernel's arithmetic operation by operation in numpy float32 (sums in double) -> v_alpha [C,H,W,1] float32"""
    f = np.float32
    a = np.asarray(alpha, f)[..., 0]
    t_bg = np.zeros_like(a)
    if b is not None:
        bb, vv = np.asarray(b, f)[:, None, None, :], np.asarray(v, f)
        # fmaf(b2, v2, fmaf(b1, v1, b0 v0)): every product and partial sum is exact on these inputs, so fused = unfused
        t_bg = -((bb[..., 0] * vv[..., 0] + bb[..., 1] * vv[..., 1]) + bb[..., 2] * vv[..., 2])
    t_a = np.zeros_like(a)
    if M is not None:
        w32 = np.asarray(w, f)
        on = w32 > 0
        n_c = np.maximum(np.where(on, w32, 0).astype(np.float64).sum((1, 2)), 1.0)
        k = (np.float64(f(alpha_fac)) / n_c).astype(f)[:, None, None]
        with np.errstate(invalid="ignore"):
            diff = np.where(on, a.astype(np.float64) - np.where(on, np.asarray(M, f), 0).astype(np.float64), 0.0)
            t_a = np.where(on, (k * np.where(on, w32, 0)) * np.sign(diff).astype(f), f(0)).astype(f)
    vin = np.zeros_like(a) if v_in is None else np.asarray(v_in, f)[..., 0]
    return ((vin + t_bg) + t_a).astype(f)[..., None]
