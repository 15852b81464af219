"""Inputs and float64 references of the activated parameterisation (csrc/gs_activation.hip: k_param_activate,
k_param_activate_bwd; scene.activations), numpy and CPU torch only, no GPU.  Used by test_host_activation.py and
test_gpu_activation.py.

    S = exp(s), O = 1 / (1 + exp(-o))                                 the activation, float64 here
    v_s = (v_S + k_s) S,  v_o = ((v_O + k_o) O) (1 - O)               its chain rule, on the STORED float32 S and O:
                                                                      float32 operation by operation (activate_bwd_f32,
                                                                      what the kernel must give bit for bit) and float64
    C (opac_fac mean O + scale_fac mean S)                            the reference's regularisers, once per view

and the end-to-end loss of a fused step on top of oracle.gs_torch_ref.render_dense and view_loss, which already take the
opacities as logits and the scales as logs in their regularisers: dense_step renders exp / sigmoid of the parameters and
hands view_loss the parameters themselves.

The kernel sizes: 1 .. 5 and 255 .. 257 (one and two accesses, the tail behind the last multiple of four), N_TWO_TRIPS, the
first N whose block partials give the finishing workgroup a second trip of its loop -- stream_grid(1, N) makes
ceil(N / 1024) workgroups up to 2048 and k_stream_finish walks them 256 at a time, so 256 * 1024 + 1 -- which also has a
last workgroup of a single Gaussian, and N_RAGGED, three full workgroups and a last one of 1024 * 3 / 4 + 3 Gaussians."""
import numpy as np

STREAM_T, STREAM_ALIGN = 256, 1024                 # per_view.h
N_TWO_TRIPS = STREAM_T * STREAM_ALIGN + 1
N_RAGGED = 3 * STREAM_ALIGN + 771
KERNEL_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, N_RAGGED, N_TWO_TRIPS)


def stream_blocks(n):
    """workgroups of stream_grid(1, n) (per_view.h)"""
    want = min((n + STREAM_ALIGN - 1) // STREAM_ALIGN, 256 * 8)
    b = max(want, 1)
    ch = (n + b - 1) // b
    ch = (ch + STREAM_ALIGN - 1) // STREAM_ALIGN * STREAM_ALIGN
    return (n + ch - 1) // ch


def kernel_inputs(n, seed=0):
    """-> dict of float32 arrays: s [n,3] in [-12, 3], o [n] in [-20, 20] with a planted +90 (last entry) and, from n = 2,
    -90 (entry (n - 1) // 2); cotangents v_S [n,3], v_O [n] (normal, scaled over six decades); k_s, k_o"""
    rng = np.random.default_rng(2100 + seed + 7 * n)
    s = rng.uniform(-12.0, 3.0, (n, 3)).astype(np.float32)
    o = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    o[n - 1] = 90.0
    if n >= 2:
        o[(n - 1) // 2] = -90.0
    v_S = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 3))).astype(np.float32)
    v_O = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    return dict(s=s, o=o, v_S=v_S, v_O=v_O, k_s=np.float32(0.0123), k_o=np.float32(0.0371))


def planted(o):
    """the saturated logits of kernel_inputs"""
    return np.abs(np.asarray(o)) == 90.0


def activate_reference(s, o):
    """float64 exp(s), sigmoid(o) of float32 inputs"""
    s, o = np.asarray(s, np.float64), np.asarray(o, np.float64)
    with np.errstate(over="ignore"):
        return np.exp(s), 1.0 / (1.0 + np.exp(-o))


def float32_of(ref):
    """float64 -> the nearest float32, as float32"""
    return np.asarray(ref, np.float64).astype(np.float32)


def ulp_error(got, ref):
    """|got - ref| in float32 ulps of ref, elementwise; ref float64 and in float32's normal range (below it the spacing of
    float32 no longer follows the value, and an ulp is not a relative measure)"""
    ref = np.asarray(ref, np.float64)
    assert np.all(np.abs(ref) >= np.finfo(np.float32).tiny)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / ulp


def activate_bwd_f32(S, O, v_S, v_O, k_s=0.0, k_o=0.0):
    """the backward kernel's arithmetic in numpy float32, one rounding per operation, in its order"""
    f = np.float32
    S, O, v_S, v_O = (np.asarray(a, f) for a in (S, O, v_S, v_O))
    v_s = ((v_S + f(k_s)).astype(f) * S).astype(f)
    t = ((v_O + f(k_o)).astype(f) * O).astype(f)
    v_o = (t * (f(1.0) - O).astype(f)).astype(f)
    return v_s, v_o


def activate_bwd_reference(S, O, v_S, v_O, k_s=0.0, k_o=0.0):
    """the same chain rule in float64"""
    S, O, v_S, v_O = (np.asarray(a, np.float64) for a in (S, O, v_S, v_O))
    return (v_S + float(k_s)) * S, (v_O + float(k_o)) * O * (1.0 - O)


def reg_constants(n_views, n, opac_fac, scale_fac):
    """(k_s, k_o) as the fused step forms them, in float32: C * scale_fac / (3 N), C * opac_fac / N"""
    f = np.float32
    return f(n_views) * f(scale_fac) / (f(3.0) * f(n)), f(n_views) * f(opac_fac) / f(n)


def regularisers(S, O, n_views, opac_fac, scale_fac):
    """C (opac_fac mean O + scale_fac mean S) of the stored float32 S [N,3] and O [N], in float64, with the float32 factors"""
    S, O = np.asarray(S, np.float64), np.asarray(O, np.float64)
    return n_views * (float(np.float32(opac_fac)) * O.sum() / O.size + float(np.float32(scale_fac)) * S.sum() / S.size)


def activated_inputs_f32(s, o):
    """float32(exp(s)), float32(sigmoid(o)) computed in float64: what the raw path is fed for the error the activation may
    at most double"""
    S, O = activate_reference(s, o)
    return float32_of(S), float32_of(O)


def visibility(g, w2c, Ks, W, H, S32=None, O32=None):
    """(vis [C,N] bool, radii [C,N], margin [C,H,W]) of the C oracle's culling for the geometry the renderer sees; S32 / O32:
    the activated scales and opacities (default: g's own, raw)"""
    from oracle import gs_oracle as go
    S32 = g["scales"] if S32 is None else S32
    O32 = g["opacities"] if O32 is None else O32
    _, _, meta = go.rasterization(g["means"], g["quats"], S32, O32, g["shN"], w2c, Ks, W, H, want_margin=True)
    N, Cn = g["means"].shape[0], w2c.shape[0]
    vis = np.zeros((Cn, N), bool); rad = np.zeros((Cn, N), np.int64)
    vis[meta["camera_ids"], meta["gaussian_ids"]] = True
    rad[meta["camera_ids"], meta["gaussian_ids"]] = meta["radii"]
    return vis, rad, meta["margin"]


def dense_render(g, w2c, Ks, W, H, vis, rad, activated, render=None):
    """float64 dense render of the float32 parameters g -> (rgb [C,H,W,3], alpha [C,H,W,1], P): P the float64 leaves
    (requires_grad) means, quats, scales, opacities, shN; activated: the renderer sees exp(P.scales), sigmoid(P.opacities).
    render: a renderer with gs_torch_ref.render_dense's arguments (default: itself); whatever it returns comes before P"""
    import torch
    from oracle import gs_torch_ref as tr
    P = {k: torch.tensor(np.asarray(g[k]), dtype=torch.float64, requires_grad=True)
         for k in ("means", "quats", "scales", "opacities", "shN")}
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    S = torch.exp(P["scales"]) if activated else P["scales"]
    O = torch.sigmoid(P["opacities"]) if activated else P["opacities"]
    out = (render or tr.render_dense)(P["means"], P["quats"], S, O, P["shN"], t(w2c), t(Ks), W, H, torch.tensor(vis),
                                      torch.tensor(rad))
    return (*out, P)


def dense_step(g, w2c, Ks, W, H, gt, vis, rad, ssim_fac, opac_fac, scale_fac):
    """one activated training step in float64: the loss of starster/gs.py:149-152 -- view_loss per view, whose regularisers
    read the parameters as logits and logs -- on the render of exp / sigmoid of the same parameters
    -> (loss float, grads dict of float64 arrays: means, quats, scales, opacities, sh [N,4,3])"""
    import torch
    from oracle import gs_torch_ref as tr
    rgb, _, P = dense_render(g, w2c, Ks, W, H, vis, rad, True)
    GT = torch.tensor(np.asarray(gt), dtype=torch.float64)
    loss = sum(tr.view_loss(rgb[c], GT[c], P["opacities"], P["scales"], float(np.float32(ssim_fac)),
                            float(np.float32(opac_fac)), float(np.float32(scale_fac))) for c in range(rgb.shape[0]))
    loss.backward()
    G = {k: P[k].grad.numpy() for k in ("means", "quats", "scales", "opacities")}
    G["sh"] = P["shN"].grad.numpy()[:, :4]
    return float(loss), G
