"""torch-tensor front-end of the C ABI (include/st3r.h).

PyTorch is plumbing here: it owns device memory and the stream; every function below hands
raw device pointers to libst3r_hip.so.  All tensors must live on the context's GPU.
"""
import ctypes as C
import math
import numbers

import torch

from . import _lib

SPLAT = 12
TILE = 16


class Context:
    """One st3r_ctx per (process, GPU): owns the grow-only scratch arena."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.St3rError(f"the st3r hot path needs a GPU device, got {device!r} (no CPU fallback)")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self._h = C.c_void_p()
        with torch.cuda.device(idx):
            _lib.check(_lib.lib().st3r_ctx_create(idx, C.byref(self._h)))
        import os
        if os.environ.get("ST3R_DEBUG_FLAGS"):   # kernel A/B switches of st3r_ctx_set_debug (tools/, profiling runs)
            _lib.check(_lib.lib().st3r_ctx_set_debug(self._h, int(os.environ["ST3R_DEBUG_FLAGS"])))

    @property
    def handle(self):
        return self._h

    def arena_bytes(self):
        return int(_lib.lib().st3r_ctx_arena_bytes(self._h))

    def release_scratch(self):
        """Give the grow-only scratch arena back to the device allocator (st3r_ctx_release_scratch); the context stays
        valid and allocates again on its next call.  Raises what `settle` would raise."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().st3r_ctx_release_scratch(self._h))

    def close(self):
        if self._h:
            _lib.lib().st3r_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts = {}


def get_context(device):
    d = torch.device(device)
    idx = d.index if d.index is not None else torch.cuda.current_device()
    if idx not in _contexts:
        _contexts[idx] = Context(torch.device("cuda", idx))
    return _contexts[idx]


def release_scratch():
    """release_scratch() of every cached per-GPU context of this process (e.g. before handing the GPU to Mast3r
    inference or to another process)."""
    for ctx in _contexts.values():
        ctx.release_scratch()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, dtype=torch.float32):
    if t is None:
        return None
    if t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"expected contiguous cuda {dtype} tensor, got {t.dtype} contiguous={t.is_contiguous()} "
                         f"device={t.device}")
    return C.c_void_p(t.data_ptr())


def _f(t):
    return t.detach().to(torch.float32).contiguous()


def tile_grid(W, H):
    return math.ceil(W / TILE), math.ceil(H / TILE)


def camera_positions(viewmats):
    """inverse(viewmats)[:, :3, 3] (gsplat: camtoworlds = torch.inverse(viewmats))."""
    return torch.inverse(viewmats)[:, :3, 3].contiguous()


def sh_stride_of(sh):
    return int(sh.numel() // sh.shape[0])


def _gaussians(params):
    """the argument run `means, quats, scales, opacities, sh, sh_stride` of the C calls, from a params dict"""
    sh = params["shN"]
    return (_p(params["means"]), _p(params["quats"]), _p(params["scales"]), _p(params["opacities"]), _p(sh),
            sh_stride_of(sh))


def _stats(stats):
    """the statistics a training call wrote (int64[4]) as a dict; None when none were asked for"""
    if stats is None:
        return None
    return dict(n_visible=int(stats[0]), n_isects=int(stats[1]), arena_bytes=int(stats[2]), n_isects_ref=int(stats[3]))


def _set_registration(ctx, name, keep, gt, payload, shapes_ok, *extra):
    """The body of set_gt_moments, set_depth_prior and set_exposure: st3r_ctx_set_<name> on (gt, *payload, C, H, W,
    *extra), or with a None among the tensors the call that clears it.  The attribute `keep` of ctx keeps the tensors alive."""
    fn = getattr(_lib.lib(), "st3r_ctx_set_" + name)
    if gt is None or any(t is None for t in payload):
        _lib.check(fn(ctx.handle, None, *(None for _ in payload), 0, 0, 0, *(0.0 for _ in extra)))
        setattr(ctx, keep, None)
        return
    assert gt.is_contiguous() and shapes_ok()
    _lib.check(fn(ctx.handle, _p(gt), *(_p(t) for t in payload), gt.shape[0], gt.shape[1], gt.shape[2], *extra))
    setattr(ctx, keep, (gt, *payload))


def project_sh(ctx, means, quats, scales, opacities, sh, viewmats, Ks, campos, W, H, reg_sums=None,
               eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0, out=None):
    """out: optional (splats [Cn*N,12], tiles int32 [Cn*N]) buffers to write into (steady-state loops)."""
    N, Cn = means.shape[0], viewmats.shape[0]
    if out is not None:
        splats, tiles = out
    else:
        splats = torch.empty((Cn * N, SPLAT), dtype=torch.float32, device=means.device)
        tiles = torch.empty((Cn * N,), dtype=torch.int32, device=means.device)
    _lib.check(_lib.lib().st3r_gs_project_sh(
        ctx.handle, _stream(), N, Cn, _p(means), _p(quats), _p(scales), _p(opacities), _p(sh), sh_stride_of(sh),
        _p(viewmats), _p(Ks), _p(campos), W, H, TILE, eps2d, near, far, radius_clip, _p(splats),
        _p(tiles, torch.int32), _p(reg_sums, torch.float64)))
    return splats, tiles


def isect_scan(ctx, tiles):
    """st3r_gs_isect_scan on its own: inclusive prefix sum of int32 counts -> (cum, total on the host)."""
    cum = torch.empty_like(tiles)
    n = C.c_int64(0)
    _lib.check(_lib.lib().st3r_gs_isect_scan(ctx.handle, _stream(), tiles.numel(), _p(tiles, torch.int32),
                                             _p(cum, torch.int32), C.byref(n)))
    return cum, n.value


def isect(ctx, splats, tiles, N, Cn, W, H):
    tw, th = tile_grid(W, H)
    cum = torch.empty_like(tiles)
    n = C.c_int64(0)
    _lib.check(_lib.lib().st3r_gs_isect_scan(ctx.handle, _stream(), N * Cn, _p(tiles, torch.int32),
                                             _p(cum, torch.int32), C.byref(n)))
    n = n.value
    ids = torch.empty((n,), dtype=torch.int64, device=splats.device)
    flat = torch.empty((n,), dtype=torch.int32, device=splats.device)
    _lib.check(_lib.lib().st3r_gs_isect_emit(ctx.handle, _stream(), N, Cn, _p(splats), _p(cum, torch.int32), TILE, tw,
                                             th, n, _p(ids, torch.int64), _p(flat, torch.int32)))
    return cum, ids, flat


def radix_sort_pairs(ctx, keys, vals, begin_bit, end_bit):
    """Stable ascending radix sort of (key, int32 value) pairs on key bits [begin_bit, end_bit).  keys: int32 or
    int64 tensor holding UNSIGNED 32/64-bit patterns; vals int32 or None.  Inputs are left untouched."""
    assert keys.dtype in (torch.int32, torch.int64)
    kb = 4 if keys.dtype == torch.int32 else 8
    ko = torch.empty_like(keys)
    vo = torch.empty_like(vals) if vals is not None else None
    _lib.check(_lib.lib().st3r_radix_sort_pairs(ctx.handle, _stream(), kb, keys.numel(), begin_bit, end_bit,
                                                _p(keys, keys.dtype), _p(vals, torch.int32), _p(ko, keys.dtype),
                                                _p(vo, torch.int32)))
    return ko, vo


def sort_pairs(ctx, ids, flat, end_bit):
    ids_in, flat_in = ids.clone(), flat.clone()
    ids_out, flat_out = torch.empty_like(ids), torch.empty_like(flat)
    _lib.check(_lib.lib().st3r_gs_sort(ctx.handle, _stream(), ids.numel(), end_bit, _p(ids_in, torch.int64),
                                       _p(flat_in, torch.int32), _p(ids_out, torch.int64),
                                       _p(flat_out, torch.int32)))
    return ids_out, flat_out


def offsets(ctx, ids_sorted, Cn, W, H):
    tw, th = tile_grid(W, H)
    off = torch.empty((Cn, th, tw), dtype=torch.int32, device=ids_sorted.device)
    _lib.check(_lib.lib().st3r_gs_offsets(ctx.handle, _stream(), ids_sorted.numel(), _p(ids_sorted, torch.int64), Cn,
                                          tw, th, _p(off, torch.int32)))
    return off


def blend_fwd(ctx, splats, off, flat, Cn, W, H):
    tw, th = tile_grid(W, H)
    dev = splats.device
    rgb = torch.empty((Cn, H, W, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((Cn, H, W, 1), dtype=torch.float32, device=dev)
    last = torch.empty((Cn, H, W), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().st3r_gs_blend_fwd(ctx.handle, _stream(), Cn, W, H, TILE, tw, th, _p(splats),
                                            _p(off, torch.int32), _p(flat, torch.int32), flat.numel(), _p(rgb),
                                            _p(alpha), _p(last, torch.int32)))
    return rgb, alpha, last


def blend_bwd(ctx, splats, off, flat, alpha, last, v_rgb, v_alpha, cum, Cn, W, H):
    tw, th = tile_grid(W, H)
    v_splats = torch.empty_like(splats)
    _lib.check(_lib.lib().st3r_gs_blend_bwd(ctx.handle, _stream(), Cn, W, H, TILE, tw, th, _p(splats),
                                            _p(off, torch.int32), _p(flat, torch.int32), flat.numel(), _p(alpha),
                                            _p(last, torch.int32), _p(v_rgb), _p(v_alpha), _p(cum, torch.int32),
                                            splats.shape[0], _p(v_splats)))
    return v_splats


def blend_depth_fwd(ctx, splats, off, flat, alpha, last, Cn, W, H):
    """Depth map [Cn,H,W,1] with the weights of the blend_fwd call that returned (alpha, last)."""
    tw, th = tile_grid(W, H)
    depth = torch.empty((Cn, H, W, 1), dtype=torch.float32, device=splats.device)
    _lib.check(_lib.lib().st3r_gs_blend_depth_fwd(ctx.handle, _stream(), Cn, W, H, TILE, tw, th, _p(splats),
                                                  _p(off, torch.int32), _p(flat, torch.int32), flat.numel(), _p(alpha),
                                                  _p(last, torch.int32), _p(depth)))
    return depth


def blend_depth_bwd(ctx, splats, off, flat, alpha, last, v_depth, cum, Cn, W, H):
    """Per-pair gradients of the depth map (floats 0-5 and 9 of v_splats); must follow blend_fwd of the same lists."""
    tw, th = tile_grid(W, H)
    v_splats = torch.empty_like(splats)
    _lib.check(_lib.lib().st3r_gs_blend_depth_bwd(ctx.handle, _stream(), Cn, W, H, TILE, tw, th, _p(splats),
                                                  _p(off, torch.int32), _p(flat, torch.int32), flat.numel(), _p(alpha),
                                                  _p(last, torch.int32), _p(v_depth), _p(cum, torch.int32),
                                                  splats.shape[0], _p(v_splats)))
    return v_splats


def depth_bwd(ctx, means, viewmats, splats, v_splats, grads, v_viewmats=None):
    """Adds the depth column of v_splats into grads[0:3N] (means) and, if given, into v_viewmats [Cn,4,4]."""
    N, Cn = means.shape[0], viewmats.shape[0]
    _lib.check(_lib.lib().st3r_gs_depth_bwd(ctx.handle, _stream(), N, Cn, _p(means), _p(viewmats), _p(splats),
                                            _p(v_splats), _p(grads), _p(v_viewmats)))
    return grads, v_viewmats


def project_sh_bwd(ctx, means, quats, scales, opacities, sh, viewmats, Ks, campos, W, H, splats, v_splats,
                   reg_views=0.0, opac_fac=0.0, scale_fac=0.0, eps2d=0.3, out=None):
    N, Cn = means.shape[0], viewmats.shape[0]
    grads = out if out is not None else torch.empty((23 * N,), dtype=torch.float32, device=means.device)
    _lib.check(_lib.lib().st3r_gs_project_sh_bwd(
        ctx.handle, _stream(), N, Cn, _p(means), _p(quats), _p(scales), _p(opacities), _p(sh), sh_stride_of(sh),
        _p(viewmats), _p(Ks), _p(campos), W, H, eps2d, _p(splats), _p(v_splats), reg_views, opac_fac, scale_fac,
        _p(grads)))
    return grads


def viewmat_bwd(ctx, means, quats, scales, sh, viewmats, Ks, campos, W, H, splats, v_splats, eps2d=0.3, out=None):
    """d loss / d viewmats [C,4,4] from the per-pair gradients of blend_bwd (gsplat's v_viewmats), including the
    view-direction term through campos = inverse(viewmats)[:, :3, 3]."""
    N, Cn = means.shape[0], viewmats.shape[0]
    v_viewmats = out if out is not None else torch.empty((Cn, 4, 4), dtype=torch.float32, device=means.device)
    _lib.check(_lib.lib().st3r_gs_viewmat_bwd(
        ctx.handle, _stream(), N, Cn, _p(means), _p(quats), _p(scales), _p(sh), sh_stride_of(sh), _p(viewmats),
        _p(Ks), _p(campos), W, H, eps2d, _p(splats), _p(v_splats), _p(v_viewmats)))
    return v_viewmats


def intrinsics_bwd(ctx, means, quats, scales, viewmats, Ks, W, H, splats, v_splats, eps2d=0.3, out=None):
    """d loss / d (fx, fy, cx, cy) [C,4] from the per-pair gradients of blend_bwd, the clamp limits' dependence on K
    included (st3r_gs_intrinsics_bwd)."""
    N, Cn = means.shape[0], viewmats.shape[0]
    v_Ks = out if out is not None else torch.empty((Cn, 4), dtype=torch.float32, device=means.device)
    _lib.check(_lib.lib().st3r_gs_intrinsics_bwd(
        ctx.handle, _stream(), N, Cn, _p(means), _p(quats), _p(scales), _p(viewmats), _p(Ks), W, H, eps2d, _p(splats),
        _p(v_splats), _p(v_Ks)))
    return v_Ks


def split_grads(grads, N):
    """views into the block layout means[3N] quats[4N] scales[3N] opacities[N] sh4[12N]"""
    return dict(means=grads[0:3 * N].view(N, 3), quats=grads[3 * N:7 * N].view(N, 4),
                scales=grads[7 * N:10 * N].view(N, 3), opacities=grads[10 * N:11 * N],
                sh=grads[11 * N:23 * N].view(N, 4, 3))


def loss_l1_ssim(ctx, render, gt, w_l1, w_ssim, want_grad=True):
    Cn, H, W = render.shape[0], render.shape[1], render.shape[2]
    sums = torch.empty((Cn, 2), dtype=torch.float64, device=render.device)
    v = torch.empty_like(render) if want_grad else None
    _lib.check(_lib.lib().st3r_loss_l1_ssim(ctx.handle, _stream(), Cn, H, W, _p(render), _p(gt), w_l1, w_ssim,
                                            _p(sums, torch.float64), _p(v)))
    return sums, v


def gt_moments(ctx, gt):
    """(conv(gt), conv(gt^2)) of SSIM's 11 x 11 window for the images gt [C,H,W,3]: [C,H,W,3,2], computed once per
    training call (st3r_loss_gt_moments)."""
    Cn, H, W = gt.shape[0], gt.shape[1], gt.shape[2]
    mom = torch.empty((Cn, H, W, 3, 2), dtype=torch.float32, device=gt.device)
    _lib.check(_lib.lib().st3r_loss_gt_moments(ctx.handle, _stream(), Cn, H, W, _p(gt), _p(mom)))
    return mom


def set_gt_moments(ctx, gt, moments):
    """Register (gt, moments) with the ctx -- the loss kernels then read the moments instead of convolving gt -- or clear
    the registration (gt = None).  The caller keeps both tensors alive and unchanged while registered."""
    _set_registration(ctx, "gt_moments", "_gtm_keep", gt, (moments,),
                      lambda: moments.is_contiguous() and moments.shape == (*gt.shape, 2))


def loss_l1_ssim_weighted(ctx, render, gt, weight, w_l1, w_ssim, want_grad=True):
    """L1 + SSIM of render against gt [C,H,W,3] under per-pixel weights [C,H,W] float32 >= 0
    (st3r_loss_l1_ssim_weighted): the weight multiplies the L1 term of its pixel and the SSIM map at the window's centre.
    Returns (sums [C,4] float64: sum_p w |gt - r|, sum_I w ssim, n1 = max(sum_p w, 1), n2 = max(sum_I w, 1) per view,
    v_render or None)."""
    Cn, H, W = render.shape[0], render.shape[1], render.shape[2]
    if tuple(weight.shape) != (Cn, H, W) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError(f"expected contiguous float32 weights {(Cn, H, W)}, got {weight.dtype} {tuple(weight.shape)}")
    sums = torch.empty((Cn, 4), dtype=torch.float64, device=render.device)
    v = torch.empty_like(render) if want_grad else None
    _lib.check(_lib.lib().st3r_loss_l1_ssim_weighted(ctx.handle, _stream(), Cn, H, W, _p(render), _p(gt), _p(weight), w_l1,
                                                     w_ssim, _p(sums, torch.float64), _p(v)))
    return sums, v


def set_loss_weight(ctx, gt, weight):
    """Register the per-pixel loss weights [C,H,W] (float32, >= 0) of the images gt [C,H,W,3] with the ctx -- train_fwd_bwd,
    train_step and train_step_poses on `gt` (or whole views of it) then take the weighted loss of loss_l1_ssim_weighted
    (st3r_ctx_set_loss_weight) -- or clear the registration (gt = None).  The caller's tensors are kept alive here and must
    stay unchanged while registered."""
    _set_registration(ctx, "loss_weight", "_lw_keep", gt, (weight,),
                      lambda: weight.is_contiguous() and weight.dtype == torch.float32 and
                      weight.shape == tuple(gt.shape[:3]))


def loss_depth_prior(ctx, depth, alpha, prior, weight, depth_fac):
    """Weighted L1 between the expected depth ED = depth / max(alpha, 1e-10) of a render (depth, alpha [C,H,W,1]) and a
    prior [C,H,W] under weights [C,H,W] >= 0 (st3r_loss_depth_prior).  Returns (sums [C,2] float64: sum_p w |ED - Z| and
    n_c = max(sum_p w, 1) per view, v_depth, v_alpha [C,H,W,1]); the loss is depth_fac * (sums[:, 0] / sums[:, 1]).sum()."""
    Cn, H, W = depth.shape[0], depth.shape[1], depth.shape[2]
    assert alpha.shape == depth.shape and prior.shape == (Cn, H, W) and weight.shape == (Cn, H, W)
    sums = torch.empty((Cn, 2), dtype=torch.float64, device=depth.device)
    v_depth, v_alpha = torch.empty_like(depth), torch.empty_like(depth)
    _lib.check(_lib.lib().st3r_loss_depth_prior(ctx.handle, _stream(), Cn, H, W, _p(depth), _p(alpha), _p(prior),
                                                _p(weight), depth_fac, _p(sums, torch.float64), _p(v_depth), _p(v_alpha)))
    return sums, v_depth, v_alpha


def set_depth_prior(ctx, gt, depth, weight, depth_fac=1.0):
    """Register a depth prior (depth, weight [C,H,W]) for the images gt [C,H,W,3] with the ctx -- train_fwd_bwd, train_step
    and train_step_poses on `gt` (or whole views of it) then add depth_fac * sum_p w |ED - Z| / max(sum_p w, 1) per view to
    their loss (st3r_ctx_set_depth_prior) -- or clear the registration (gt = None).  The caller's tensors are kept alive
    here and must stay unchanged while registered."""
    _set_registration(ctx, "depth_prior", "_dp_keep", gt, (depth, weight),
                      lambda: depth.shape == tuple(gt.shape[:3]) and weight.shape == tuple(gt.shape[:3]), float(depth_fac))


def _exposure_shapes(rgb, exposure):
    if rgb.dim() != 4 or rgb.shape[-1] != 3 or tuple(exposure.shape) != (rgb.shape[0], 3, 4):
        raise ValueError(f"expected images [C,H,W,3] and exposures [C,3,4], got {tuple(rgb.shape)} and "
                         f"{tuple(exposure.shape)}")
    return rgb.shape[0], rgb.shape[1], rgb.shape[2]


def exposure_fwd(ctx, rgb, exposure, out=None):
    """y = A x + t per pixel of rgb [C,H,W,3] with the view's exposure [C,3,4] = [A | t] (st3r_exposure_fwd)."""
    Cn, H, W = _exposure_shapes(rgb, exposure)
    out = torch.empty_like(rgb) if out is None else out
    _lib.check(_lib.lib().st3r_exposure_fwd(ctx.handle, _stream(), Cn, H, W, _p(rgb), _p(exposure), _p(out)))
    return out


def exposure_bwd(ctx, rgb, exposure, v_out, v_rgb=None, v_exposure=None):
    """Backward of exposure_fwd from v_out = d loss / d y; rgb is the forward's input.  Returns (v_rgb [C,H,W,3],
    v_exposure [C,3,4]); v_rgb may be v_out itself (in place) (st3r_exposure_bwd)."""
    Cn, H, W = _exposure_shapes(rgb, exposure)
    if v_out.shape != rgb.shape:
        raise ValueError(f"v_out has shape {tuple(v_out.shape)}, the images {tuple(rgb.shape)}")
    v_rgb = torch.empty_like(rgb) if v_rgb is None else v_rgb
    v_exposure = torch.empty_like(exposure) if v_exposure is None else v_exposure
    _lib.check(_lib.lib().st3r_exposure_bwd(ctx.handle, _stream(), Cn, H, W, _p(rgb), _p(exposure), _p(v_out), _p(v_rgb),
                                            _p(v_exposure)))
    return v_rgb, v_exposure


def exposure_adam_step(ctx, exposure, v_exposure, m, v, lr, b1, b2, eps, step, mask=None):
    """One Adam step on the exposures [C,3,4], in place, from v_exposure [C,3,4]; moments m / v [12C]
    (st3r_exposure_adam_step).  mask [C] floats or None: views with mask == 0 keep every bit."""
    Cn = exposure.shape[0]
    assert exposure.numel() == 12 * Cn and v_exposure.numel() == 12 * Cn and m.numel() == 12 * Cn and v.numel() == 12 * Cn
    _lib.check(_lib.lib().st3r_exposure_adam_step(ctx.handle, _stream(), Cn, _p(exposure), _p(v_exposure), _p(m), _p(v), lr,
                                                  b1, b2, eps, step, _p(mask)))


def set_exposure(ctx, gt, exposure, v_exposure):
    """Register the exposures [C,3,4] of the images gt [C,H,W,3] and the buffer v_exposure [C,3,4] that receives their
    gradient -- train_fwd_bwd, train_step and train_step_poses on `gt` (or whole views of it) then compare the exposed
    render with the ground truth and write v_exposure (st3r_ctx_set_exposure) -- or clear the registration (gt = None).
    The caller's tensors are kept alive here."""
    _set_registration(ctx, "exposure", "_ex_keep", gt, (exposure, v_exposure),
                      lambda: tuple(exposure.shape) == (gt.shape[0], 3, 4) and v_exposure.shape == exposure.shape)


def _alpha_shapes(alpha, backgrounds=None, **images):
    """(C, H, W) of alpha [C,H,W,1]; ValueError unless backgrounds is [C,3], every named image [C,H,W,3] or, for a name
    ending in `map`, [C,H,W] -- float32 all of them (None entries are skipped)"""
    if alpha.dim() != 4 or alpha.shape[-1] != 1 or alpha.dtype != torch.float32:
        raise ValueError(f"expected float32 alpha [C,H,W,1], got {alpha.dtype} {tuple(alpha.shape)}")
    Cn, H, W = alpha.shape[:3]
    if backgrounds is not None and (tuple(backgrounds.shape) != (Cn, 3) or backgrounds.dtype != torch.float32):
        raise ValueError(f"expected float32 backgrounds ({Cn}, 3), got {backgrounds.dtype} {tuple(backgrounds.shape)}")
    for name, t in images.items():
        want = (Cn, H, W) if name.endswith("map") else ((Cn, H, W, 1) if name.startswith("v_alpha") else (Cn, H, W, 3))
        if t is not None and (tuple(t.shape) != want or t.dtype != torch.float32):
            raise ValueError(f"expected float32 {name} {want}, got {t.dtype} {tuple(t.shape)}")
    return Cn, H, W


def composite_fwd(ctx, rgb, alpha, backgrounds, out=None):
    """The render rgb [C,H,W,3] with accumulated opacity alpha [C,H,W,1] over the views' background colours [C,3]:
    y = x + (1 - alpha) b per pixel (st3r_composite_fwd).  out may be rgb itself (in place)."""
    Cn, H, W = _alpha_shapes(alpha, backgrounds, rgb=rgb, out=out)
    out = torch.empty_like(rgb) if out is None else out
    _lib.check(_lib.lib().st3r_composite_fwd(ctx.handle, _stream(), Cn, H, W, _p(rgb), _p(alpha), _p(backgrounds), _p(out)))
    return out


def alpha_grad(ctx, alpha, backgrounds=None, v_out=None, target=None, weight=None, alpha_fac=0.0, v_alpha_in=None,
               v_alpha=None, want_v_backgrounds=False):
    """d loss / d alpha of a render [C,H,W,1] besides the depth prior's, in one pass (st3r_alpha_grad).  Background term
    (backgrounds [C,3] and v_out = d loss / d composite [C,H,W,3]): -sum_j b_j v_j, and with want_v_backgrounds
    v_backgrounds [C,3] = sum_p (1 - alpha) v.  Alpha term (target, weight [C,H,W], alpha_fac): the derivative of
    alpha_fac * sum_p w |alpha - target| / max(sum_p w, 1) per view.  v_alpha_in: added first; v_alpha (output) may be
    v_alpha_in itself.  Returns (v_alpha, sums [C,2] float64 -- sum_p w |alpha - target| and n_c -- or None,
    v_backgrounds or None)."""
    Cn, H, W = _alpha_shapes(alpha, backgrounds, v_out=v_out, target_map=target, weight_map=weight, v_alpha_in=v_alpha_in,
                             v_alpha=v_alpha)
    if (backgrounds is None) != (v_out is None) or (target is None) != (weight is None):
        raise ValueError("a term is given whole: backgrounds with v_out, target with weight")
    if backgrounds is None and target is None:
        raise ValueError("alpha_grad needs the background term, the alpha term or both")
    v_alpha = torch.empty_like(alpha) if v_alpha is None else v_alpha
    sums = torch.empty((Cn, 2), dtype=torch.float64, device=alpha.device) if target is not None else None
    v_b = torch.empty((Cn, 3), dtype=torch.float32, device=alpha.device) if want_v_backgrounds and backgrounds is not None \
        else None
    _lib.check(_lib.lib().st3r_alpha_grad(ctx.handle, _stream(), Cn, H, W, _p(alpha), _p(backgrounds), _p(v_out), _p(target),
                                          _p(weight), float(alpha_fac), _p(v_alpha_in), _p(sums, torch.float64), _p(v_alpha),
                                          _p(v_b)))
    return v_alpha, sums, v_b


def set_background(ctx, gt, backgrounds):
    """Register the background colours [C,3] (float32) of the images gt [C,H,W,3] with the ctx -- train_fwd_bwd, train_step
    and train_step_poses on `gt` (or whole views of it) then compare the render composited over them with the ground truth
    (st3r_ctx_set_background) -- or clear the registration (gt = None).  The caller's tensors are kept alive here."""
    _set_registration(ctx, "background", "_bg_keep", gt, (backgrounds,),
                      lambda: backgrounds.is_contiguous() and backgrounds.dtype == torch.float32 and
                      tuple(backgrounds.shape) == (gt.shape[0], 3))


def set_alpha_target(ctx, gt, target, weight, alpha_fac=1.0):
    """Register alpha targets (target, weight [C,H,W] float32) for the images gt [C,H,W,3] with the ctx -- train_fwd_bwd,
    train_step and train_step_poses on `gt` (or whole views of it) then add alpha_fac * sum_p w |alpha - target| /
    max(sum_p w, 1) per view to their loss (st3r_ctx_set_alpha_target) -- or clear the registration (gt = None).  The
    caller's tensors are kept alive here and must stay unchanged while registered."""
    _set_registration(ctx, "alpha_target", "_at_keep", gt, (target, weight),
                      lambda: all(t.is_contiguous() and t.dtype == torch.float32 and t.shape == tuple(gt.shape[:3])
                                  for t in (target, weight)), float(alpha_fac))


def _activation_shapes(scales, **others):
    """N of scales [N,3]; ValueError unless every named tensor has scales' shape or, for a name ending in `opacities`, [N]
    -- float32 all of them"""
    if scales.dim() != 2 or scales.shape[1] != 3 or scales.dtype != torch.float32:
        raise ValueError(f"expected float32 scales [N,3], got {scales.dtype} {tuple(scales.shape)}")
    N = scales.shape[0]
    for name, t in others.items():
        want = (N,) if name.endswith("opacities") else (N, 3)
        if t is not None and (tuple(t.shape) != want or t.dtype != torch.float32):
            raise ValueError(f"expected float32 {name} {want}, got {t.dtype} {tuple(t.shape)}")
    return N


def param_activate(ctx, scales, opacities, act_scales=None, act_opacities=None, want_sums=False):
    """exp(scales) [N,3] and sigmoid(opacities) [N] of log-scales and logits (st3r_param_activate).  want_sums: also
    float64 [2] = (sum sigmoid, sum exp) of the stored float32 values.  Returns (act_scales, act_opacities, sums or None)."""
    N = _activation_shapes(scales, opacities=opacities, act_scales=act_scales, act_opacities=act_opacities)
    act_scales = torch.empty_like(scales) if act_scales is None else act_scales
    act_opacities = torch.empty_like(opacities) if act_opacities is None else act_opacities
    sums = torch.empty(2, dtype=torch.float64, device=scales.device) if want_sums else None
    _lib.check(_lib.lib().st3r_param_activate(ctx.handle, _stream(), N, _p(scales), _p(opacities), _p(act_scales),
                                              _p(act_opacities), _p(sums, torch.float64)))
    return act_scales, act_opacities, sums


def param_activate_bwd(ctx, act_scales, act_opacities, v_act_scales, v_act_opacities, reg_s_k=0.0, reg_o_k=0.0,
                       v_scales=None, v_opacities=None):
    """The chain rule of param_activate on its stored outputs: v_scales = (v_act_scales + reg_s_k) * act_scales,
    v_opacities = (v_act_opacities + reg_o_k) * act_opacities * (1 - act_opacities) (st3r_param_activate_bwd).  The
    outputs may be v_act_scales / v_act_opacities themselves (in place).  Returns (v_scales, v_opacities)."""
    N = _activation_shapes(act_scales, act_opacities=act_opacities, v_act_scales=v_act_scales,
                           v_act_opacities=v_act_opacities, v_scales=v_scales, v_opacities=v_opacities)
    v_scales = torch.empty_like(act_scales) if v_scales is None else v_scales
    v_opacities = torch.empty_like(act_opacities) if v_opacities is None else v_opacities
    _lib.check(_lib.lib().st3r_param_activate_bwd(ctx.handle, _stream(), N, _p(act_scales), _p(act_opacities),
                                                  _p(v_act_scales), _p(v_act_opacities), float(reg_s_k), float(reg_o_k),
                                                  _p(v_scales), _p(v_opacities)))
    return v_scales, v_opacities


def set_activation(ctx, on):
    """Whether train_fwd_bwd, train_step, train_step_poses and render read `scales` as log-scales and `opacities` as logits
    from now on (a setting of the ctx, st3r_ctx_set_activation).  Returns the previous setting."""
    prev = get_activation(ctx)
    _lib.check(_lib.lib().st3r_ctx_set_activation(ctx.handle, 1 if on else 0))
    return prev


def get_activation(ctx):
    on = C.c_int(-1)
    _lib.check(_lib.lib().st3r_ctx_get_activation(ctx.handle, C.byref(on)))
    return bool(on.value)


SH_DEFAULT = (1, 1, None)


def sh_rows(degree):
    """rows of an SH tensor of this degree"""
    return (degree + 1) ** 2


def set_sh_degree(ctx, degree, active_degree=None, v_sh_high=None):
    """The SH degree every call that evaluates SH uses from now on (a setting of the ctx, st3r_ctx_set_sh_degree):
    project_sh, project_sh_bwd, viewmat_bwd, render and the training calls read sh_rows(active_degree) rows of `sh`; the
    backward calls leave the gradients of the rows 4.. in v_sh_high [N, 3 (sh_rows(degree) - 4)] (needed by them for
    degree >= 2, kept alive here).  active_degree None: degree.  Returns the previous setting, a tuple that
    set_sh_degree(ctx, *prev) restores; a ctx starts at SH_DEFAULT."""
    if isinstance(degree, bool) or not isinstance(degree, numbers.Integral) or not 0 <= degree <= 3:
        raise ValueError(f"sh degree must be an int 0..3, got {degree!r}")
    active = degree if active_degree is None else active_degree
    if isinstance(active, bool) or not isinstance(active, numbers.Integral) or not 0 <= active <= degree:
        raise ValueError(f"active sh degree must be an int 0..{degree}, got {active!r}")
    degree, active = int(degree), int(active)
    address = isinstance(v_sh_high, int)   # (what get_sh_degree returns for a buffer set behind this module's back)
    if v_sh_high is not None and not address:
        if degree < 2:
            raise ValueError("v_sh_high belongs to sh degree 2 or 3")
        if v_sh_high.dim() != 2 or v_sh_high.shape[1] != 3 * (sh_rows(degree) - 4):
            raise ValueError(f"v_sh_high must be [N, {3 * (sh_rows(degree) - 4)}], got {tuple(v_sh_high.shape)}")
    prev = get_sh_degree(ctx)
    _lib.check(_lib.lib().st3r_ctx_set_sh_degree(ctx.handle, degree, active,
                                                 C.c_void_p(v_sh_high) if address else _p(v_sh_high)))
    ctx._sh_keep = None if address else v_sh_high
    return prev


def get_sh_degree(ctx):
    """(degree, active_degree, v_sh_high) of the ctx (st3r_ctx_get_sh_degree).  v_sh_high is the tensor set_sh_degree keeps
    alive when the context still points at it, None for a NULL pointer, and the bare address (an int) of a buffer that
    was set behind this module's back."""
    if not hasattr(ctx, "handle"):       # a stand-in without a library context: the default, as a context starts
        return SH_DEFAULT
    d, a, p = C.c_int(-1), C.c_int(-1), C.c_void_p()
    _lib.check(_lib.lib().st3r_ctx_get_sh_degree(ctx.handle, C.byref(d), C.byref(a), C.byref(p)))
    kept = getattr(ctx, "_sh_keep", None)
    if not p.value:
        v = None
    else:
        v = kept if kept is not None and kept.data_ptr() == p.value else int(p.value)
    return d.value, a.value, v


def sh_high_adam_step(ctx, sh, degree, v_sh_high, m, v, lr, b1, b2, eps, step):
    """One Adam step on the rows 4 .. sh_rows(degree) - 1 of sh [N, rows, 3], in place, from v_sh_high; moments m, v
    [N, 3 (sh_rows(degree) - 4)] (st3r_sh_high_adam_step).  Guarded on the device like adam_step."""
    N, H = sh.shape[0], 3 * (sh_rows(degree) - 4)
    assert degree in (2, 3) and all(tuple(t.shape) == (N, H) for t in (v_sh_high, m, v))
    _lib.check(_lib.lib().st3r_sh_high_adam_step(ctx.handle, _stream(), N, _p(sh), sh_stride_of(sh), degree,
                                                 _p(v_sh_high), _p(m), _p(v), lr, b1, b2, eps, step))


def intrinsics_adam_step(ctx, Ks, v_Ks, k_m, k_v, lr, b1, b2, eps, step, mask, W, H, tie_focal=True, opt_pp=False):
    """One Adam step on the intrinsics Ks [C,3,3], in place, from v_Ks [C,4] = d loss / d (fx, fy, cx, cy); moments
    k_m / k_v [4C]; the parameters are (log fx, log fy, cx / W, cy / H) (st3r_intrinsics_adam_step).  tie_focal: one
    focal scalar per view (moment slot 0; fx / fy is kept); opt_pp: the principal point is trained too.  mask [C] floats
    or None: views with mask == 0 keep every bit."""
    Cn = Ks.shape[0]
    assert tuple(Ks.shape) == (Cn, 3, 3) and v_Ks.numel() == 4 * Cn and k_m.numel() == 4 * Cn and k_v.numel() == 4 * Cn
    _lib.check(_lib.lib().st3r_intrinsics_adam_step(ctx.handle, _stream(), Cn, _p(Ks), _p(v_Ks), _p(k_m), _p(k_v), lr, b1,
                                                    b2, eps, step, _p(mask), W, H,
                                                    (1 if tie_focal else 0) | (2 if opt_pp else 0)))


def set_intrinsics_grad(ctx, gt, v_Ks):
    """Register the buffer v_Ks [C,4] that receives d loss / d (fx, fy, cx, cy) of the images gt [C,H,W,3] --
    train_fwd_bwd, train_step and train_step_poses on `gt` (or whole views of it) then write it
    (st3r_ctx_set_intrinsics_grad) -- or clear the registration (gt = None).  The caller's tensors are kept alive here."""
    _set_registration(ctx, "intrinsics_grad", "_kg_keep", gt, (v_Ks,),
                      lambda: v_Ks.is_contiguous() and tuple(v_Ks.shape) == (gt.shape[0], 4))


def adam_step(ctx, params, grads, m, v, lr, b1, b2, eps, step):
    """params: dict with means, quats, scales, opacities, shN (updated in place)."""
    N = params["means"].shape[0]
    _lib.check(_lib.lib().st3r_adam_step(ctx.handle, _stream(), N, *_gaussians(params), _p(grads), _p(m), _p(v), lr, b1,
                                         b2, eps, step))


def train_fwd_bwd(ctx, params, viewmats, Ks, campos, gt, W, H, ssim_fac, opac_fac, scale_fac, grads, loss_out,
                  want_stats=True):
    """want_stats=False: see train_step."""
    N, Cn = params["means"].shape[0], viewmats.shape[0]
    stats = (C.c_int64 * 4)() if want_stats else None
    _lib.check(_lib.lib().st3r_gs_train_fwd_bwd(
        ctx.handle, _stream(), N, Cn, *_gaussians(params), _p(viewmats), _p(Ks), _p(campos), _p(gt), W, H, ssim_fac,
        opac_fac, scale_fac, _p(grads), _p(loss_out), stats))
    return _stats(stats)


def adam_step_range(ctx, params, grads, m, v, lr, b1, b2, eps, step, i0, i1, stage=None):
    """Adam on the scalars [i0, i1) of the 23N-float buffers (the piece a rank owns after a reduce-scatter); `stage`
    (23N floats, buffer order) receives the new parameter values of the piece."""
    N = params["means"].shape[0]
    _lib.check(_lib.lib().st3r_adam_step_range(
        ctx.handle, _stream(), N, *_gaussians(params), _p(grads), _p(m), _p(v), lr, b1, b2, eps, step, int(i0), int(i1),
        _p(stage)))


def params_from_stage(ctx, params, stage, i0, i1, limit):
    """parameters of the scalars outside [i0, i1) and below `limit` <- stage (buffer order)."""
    N = params["means"].shape[0]
    _lib.check(_lib.lib().st3r_params_from_stage(ctx.handle, _stream(), N, *_gaussians(params), _p(stage), int(i0),
                                                 int(i1), int(limit)))


def train_step(ctx, params, viewmats, Ks, campos, gt, W, H, ssim_fac, opac_fac, scale_fac, grads, m, v, lr, b1, b2, eps,
               step, loss_out, want_stats=True):
    """One whole iteration in one C call: fwd/bwd -> gradient all-reduce over the ctx's RCCL communicator (if
    one is attached, see dist.attach_native_comm) -> Adam.  loss_out gets this rank's part of the loss.
    want_stats=False: no statistics come back and the call does not synchronise with the device in steady state (the
    record count stays on the device; see st3r_gs_train_fwd_bwd in include/st3r.h)."""
    N, Cn = params["means"].shape[0], viewmats.shape[0]
    stats = (C.c_int64 * 4)() if want_stats else None
    _lib.check(_lib.lib().st3r_gs_train_step(
        ctx.handle, _stream(), N, Cn, *_gaussians(params), _p(viewmats), _p(Ks), _p(campos), _p(gt), W, H, ssim_fac,
        opac_fac, scale_fac, _p(grads), _p(m), _p(v), lr, b1, b2, eps, step, _p(loss_out), stats))
    return _stats(stats)


def pose_adam_step(ctx, viewmats, campos, v_viewmats, pose_m, pose_v, lr, b1, b2, eps, step, mask=None):
    """One Adam step on the cameras, in place: viewmats [C,4,4], campos [C,3], moments pose_m / pose_v [6C] (omega first),
    from v_viewmats [C,4,4]; left perturbation exp(xi^) V, rows re-orthonormalised (st3r_pose_adam_step).  mask [C]
    floats or None: cameras with mask == 0 keep every bit."""
    Cn = viewmats.shape[0]
    _lib.check(_lib.lib().st3r_pose_adam_step(ctx.handle, _stream(), Cn, _p(viewmats), _p(campos), _p(v_viewmats),
                                              _p(pose_m), _p(pose_v), lr, b1, b2, eps, step, _p(mask)))


def train_step_poses(ctx, params, viewmats, Ks, campos, gt, W, H, ssim_fac, opac_fac, scale_fac, grads, m, v, lr, b1, b2,
                     eps, step, loss_out, pose_m, pose_v, pose_lr, pose_step, pose_mask=None, v_viewmats_out=None,
                     want_stats=True):
    """train_step on a single replica that also moves the cameras: viewmats and campos are updated IN PLACE by one Adam
    step (pose_lr, the Gaussians' betas and eps, pose_step; moments pose_m / pose_v [6C]) after the Gaussians' update; both
    gradients belong to the poses the call started with.  pose_mask [C] floats: 0 freezes a camera.  v_viewmats_out
    [C,4,4]: receives this step's pose gradient.  want_stats as in train_step."""
    N, Cn = params["means"].shape[0], viewmats.shape[0]
    stats = (C.c_int64 * 4)() if want_stats else None
    _lib.check(_lib.lib().st3r_gs_train_step_poses(
        ctx.handle, _stream(), N, Cn, *_gaussians(params), _p(viewmats), _p(Ks), _p(campos), _p(gt), W, H, ssim_fac,
        opac_fac, scale_fac, _p(grads), _p(m), _p(v), lr, b1, b2, eps, step, _p(loss_out), stats, _p(pose_m), _p(pose_v),
        pose_lr, pose_step, _p(pose_mask), _p(v_viewmats_out)))
    return _stats(stats)


def dense_unproject(ctx, view_start, pixels, idxs, offsets, core, cam_rows, base_focals):
    """All dense pixels of all views (concatenated) -> world points [n,3] and own-camera depth [n]."""
    n, Cn, G = pixels.shape[0], cam_rows.shape[0], core.shape[1]
    pts = torch.empty((n, 3), dtype=torch.float32, device=cam_rows.device)
    z = torch.empty((n,), dtype=torch.float32, device=cam_rows.device)
    _lib.check(_lib.lib().st3r_dense_unproject(ctx.handle, _stream(), Cn, G, n, _p(view_start, torch.int32), _p(pixels),
                                               _p(idxs, torch.int32), _p(offsets), _p(core), _p(cam_rows),
                                               _p(base_focals), _p(pts), _p(z)))
    return pts, z


def dense_clean(ctx, view_start, sizes_hw, cam_rows, pts, zcam, conf, tol=0.001, bad_conf=0.0):
    """dust3r clean_pointcloud on the concatenated views; returns the cleaned confidences (new tensor)."""
    out = conf.clone()
    mx = int((sizes_hw[:, 0].long() * sizes_hw[:, 1].long()).max())
    _lib.check(_lib.lib().st3r_dense_clean(ctx.handle, _stream(), cam_rows.shape[0], mx, _p(view_start, torch.int32),
                                           _p(sizes_hw, torch.int32), _p(cam_rows), _p(pts), _p(zcam), tol, bad_conf,
                                           _p(out)))
    return out


def canon_view(ctx, ptmaps, confs, subsample):
    """Mast3r canonical_view(mode='avg-angle') [U]: ptmaps [n,H,W,3], confs [n,H,W] -> canon [H,W,3], canon2 [H,W],
    cconf [H,W]."""
    n, H, W = confs.shape
    canon = torch.empty((H, W, 3), device=confs.device); canon2 = torch.empty((H, W), device=confs.device)
    cconf = torch.empty((H, W), device=confs.device)
    _lib.check(_lib.lib().st3r_canon_view(ctx.handle, _stream(), n, H, W, subsample, _p(ptmaps), _p(confs), _p(canon),
                                          _p(canon2), _p(cconf)))
    return canon, canon2, cconf


def focal_weiszfeld(ctx, canon, pp, min_focal=0.5, max_focal=3.5):
    """dust3r estimate_focal_knowing_depth(focal_mode='weiszfeld') [U] -> tensor [1] on the device."""
    H, W = canon.shape[:2]
    out = torch.empty(1, device=canon.device)
    _lib.check(_lib.lib().st3r_focal_weiszfeld(ctx.handle, _stream(), H, W, _p(canon), float(pp[0]), float(pp[1]),
                                               min_focal, max_focal, _p(out)))
    return out


def focal_weiszfeld_batch(ctx, canons, pp, min_focal=0.5, max_focal=3.5):
    """The same for a stack of images of one size in one launch: canons [n,H,W,3] -> tensor [n]."""
    n, H, W = canons.shape[:3]
    out = torch.empty(n, device=canons.device)
    _lib.check(_lib.lib().st3r_focal_weiszfeld_batch(ctx.handle, _stream(), n, H, W, _p(canons), float(pp[0]),
                                                     float(pp[1]), min_focal, max_focal, _p(out)))
    return out


def focal_plan(ctx, n_views, H, W):
    """Workgroups per view that focal_weiszfeld_batch launches for n_views images of H x W on this device."""
    G = C.c_int(0)
    _lib.check(_lib.lib().st3r_focal_plan(ctx.handle, n_views, H, W, C.byref(G)))
    return G.value


def anchor_offsets(ctx, canon2, xy, subsample):
    """Mast3r anchor_depth_offsets [U] for one list of correspondence pixels xy [n,2] -> (idx int32 [n], off [n])."""
    H, W = canon2.shape
    n = xy.shape[0]
    idx = torch.empty(n, dtype=torch.int32, device=canon2.device); off = torch.empty(n, device=canon2.device)
    _lib.check(_lib.lib().st3r_anchor_offsets(ctx.handle, _stream(), n, H, W, subsample, _p(canon2), _p(xy),
                                              _p(idx, torch.int32), _p(off)))
    return idx, off


def raster_train(ctx, records, N, Cn, gt, W, H, ssim_fac, v_records, loss_out):
    """Middle phase of the Gaussian-sharded mode: records [Cn*N,12] of ALL Gaussians for this rank's views ->
    v_records (same shape), this rank's image loss."""
    stats = (C.c_int64 * 4)()
    _lib.check(_lib.lib().st3r_gs_raster_train(ctx.handle, _stream(), N, Cn, _p(records), _p(gt), W, H, ssim_fac,
                                               _p(v_records), _p(loss_out), stats))
    return dict(n_isects=int(stats[1]), arena_bytes=int(stats[2]))


def mcmc_relocate(ctx, params, m, v, min_opacity, seed, step, want_count=True):
    """In place on params (means, quats, scales, opacities, sh0 or None, shN) and on the fused Adam moments
    m, v ([23N] blocks, or None).  Returns the number of relocated Gaussians (None if not wanted: no sync)."""
    N = params["means"].shape[0]
    sh = params["shN"]; sh0 = params.get("sh0")
    n_dead = C.c_int64(0)
    _lib.check(_lib.lib().st3r_mcmc_relocate(
        ctx.handle, _stream(), N, _p(params["means"]), _p(params["quats"]), _p(params["scales"]),
        _p(params["opacities"]), None if sh0 is None else _p(sh0), _p(sh), sh_stride_of(sh),
        None if m is None else _p(m), None if v is None else _p(v), min_opacity, seed, step,
        C.byref(n_dead) if want_count else None))
    return int(n_dead.value) if want_count else None


def mcmc_add(ctx, params, N, n_new, min_opacity, seed, step):
    """params hold N + n_new rows; rows [N, N + n_new) are filled in place."""
    sh = params["shN"]; sh0 = params.get("sh0")
    assert params["means"].shape[0] >= N + n_new
    _lib.check(_lib.lib().st3r_mcmc_add(
        ctx.handle, _stream(), N, n_new, _p(params["means"]), _p(params["quats"]), _p(params["scales"]),
        _p(params["opacities"]), None if sh0 is None else _p(sh0), _p(sh), sh_stride_of(sh), min_opacity, seed, step))


def mcmc_noise(ctx, params, scaler, seed, step, row_offset=0):
    """row_offset: global row of params' first Gaussian (a shard of the set draws the noise of its own rows)."""
    N = params["means"].shape[0]
    _lib.check(_lib.lib().st3r_mcmc_noise_rows(ctx.handle, _stream(), N, int(row_offset), _p(params["means"]),
                                               _p(params["quats"]), _p(params["scales"]), _p(params["opacities"]),
                                               scaler, seed, step))


def peek(ctx, which, count, dtype=torch.int32):
    """Copy `count` elements of a ctx scratch buffer (see st3r_ctx_peek) into a new tensor (tests only)."""
    out = torch.empty((count,), dtype=dtype, device=ctx.device)
    _lib.check(_lib.lib().st3r_ctx_peek(ctx.handle, _stream(), which, _p(out, dtype), out.numel() * out.element_size()))
    return out


EXCHANGE_FORMS = ("allreduce", "ranges", "rs_ag", "direct")   # ST3R_EXCHANGE_* of include/st3r.h, in order


def set_exchange(ctx, form):
    """The form the gradient exchange inside train_step takes from now on (a setting of the ctx; all ranks must agree):
    'allreduce' | 'ranges' | 'rs_ag' | 'direct' (csrc/comm.hip).  Returns the previous form."""
    prev = get_exchange(ctx)
    _lib.check(_lib.lib().st3r_comm_set_exchange(ctx.handle, EXCHANGE_FORMS.index(form)))
    return prev


def get_exchange(ctx):
    f = C.c_int(-1)
    _lib.check(_lib.lib().st3r_comm_get_exchange(ctx.handle, C.byref(f)))
    return EXCHANGE_FORMS[f.value]


def allgather_pieces(ctx, buf):
    """In-place all-gather of the ranks' pieces of a [23N] buffer (the partition of the 'rs_ag' exchange): replicates
    Adam moments that were maintained piece-wise.  No-op without a communicator."""
    _lib.check(_lib.lib().st3r_comm_allgather_pieces(ctx.handle, _stream(), _p(buf), buf.numel()))


def settle(ctx):
    """Wait for the record count of the last asynchronous training step; raises St3rError (code -3) if that step outgrew
    its buffers (its Adam update was skipped on the device), code -5 if the last exchanged step failed on another rank
    (no rank applied it)."""
    _lib.check(_lib.lib().st3r_ctx_settle(ctx.handle))


def set_debug(ctx, flags):
    """bit 0: blend forward without the per-quadrant relevance test (tests only)."""
    _lib.check(_lib.lib().st3r_ctx_set_debug(ctx.handle, int(flags)))


def debug_set_stamps(ctx, colour=-1, depth=-1):
    """tests only: where the stamp counters of the colour / depth backward slots stand (st3r_ctx_debug_set_stamps); a
    negative value leaves that counter alone."""
    _lib.check(_lib.lib().st3r_ctx_debug_set_stamps(ctx.handle, int(colour), int(depth)))


STAGES = ("project", "scan", "emit", "sort", "offsets", "blend_fwd", "loss", "blend_bwd", "project_bwd", "adam",
          "sort_depth")


def set_profiling(ctx, enable, only=None):
    """HIP-event timing of the stages of the fused steps; `only` = a stage name: time just that stage."""
    code = 0 if not enable else (1 if only is None else 2 + STAGES.index(only))
    _lib.check(_lib.lib().st3r_ctx_set_profiling(ctx.handle, code))


def stage_ms(ctx):
    """-> {stage: (total_ms, samples)} accumulated since the last call (synchronises the device)."""
    n = 11  # ST3R_NUM_STAGES
    ms = (C.c_double * n)(); cnt = (C.c_int64 * n)()
    _lib.check(_lib.lib().st3r_ctx_get_stage_ms(ctx.handle, ms, cnt))
    return {_lib.lib().st3r_stage_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}


def render(ctx, params, viewmats, Ks, campos, W, H):
    N, Cn = params["means"].shape[0], viewmats.shape[0]
    dev = params["means"].device
    rgb = torch.empty((Cn, H, W, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((Cn, H, W, 1), dtype=torch.float32, device=dev)
    stats = (C.c_int64 * 4)()
    _lib.check(_lib.lib().st3r_gs_render(ctx.handle, _stream(), N, Cn, *_gaussians(params), _p(viewmats), _p(Ks),
                                         _p(campos), W, H, _p(rgb), _p(alpha), stats))
    return rgb, alpha, dict(n_isects=int(stats[1]))


def rasterization(ctx, means, quats, scales, opacities, colors, viewmats, Ks, width, height, want_info=True):
    """Stage-by-stage rasterization with caller-owned outputs and the gsplat-style `info` dict
    (packed arrays, reference call: starster/gs.py:76-87).  Used by Scene.render_3dgs and tests."""
    N, Cn = means.shape[0], viewmats.shape[0]
    W, H = width, height
    campos = camera_positions(viewmats)
    splats, tiles = project_sh(ctx, means, quats, scales, opacities, colors, viewmats, Ks, campos, W, H)
    cum, ids, flat = isect(ctx, splats, tiles, N, Cn, W, H)
    tw, th = tile_grid(W, H)
    end_bit = 32 + (tw * th).bit_length() + Cn.bit_length()
    ids_s, flat_s = sort_pairs(ctx, ids, flat, end_bit)
    off = offsets(ctx, ids_s, Cn, W, H)
    rgb, alpha, last = blend_fwd(ctx, splats, off, flat_s, Cn, W, H)
    info = None
    if want_info:
        radii_dense = splats[:, 10].view(torch.int32)
        vis = radii_dense > 0
        pid = torch.nonzero(vis).reshape(-1)
        packed_of_dense = torch.cumsum(vis.to(torch.int64), 0) - 1
        sp = splats[pid]
        info = dict(
            camera_ids=torch.div(pid, N, rounding_mode="floor").to(torch.int32), gaussian_ids=(pid % N).to(torch.int32),
            radii=radii_dense[pid], means2d=sp[:, 0:2], depths=sp[:, 9], conics=sp[:, 3:6], opacities=sp[:, 2],
            colors=sp[:, 6:9], tile_width=tw, tile_height=th, tiles_per_gauss=tiles[pid], isect_ids=ids_s,
            flatten_ids=packed_of_dense[flat_s.long()].to(torch.int32), isect_offsets=off, width=W, height=H,
            tile_size=TILE, n_cameras=Cn,
            # dense-id extras used by the backward / tests
            _splats=splats, _flatten_ids_dense=flat_s, _last_ids=last, _isect_ids_unsorted=ids,
            _flatten_ids_dense_unsorted=flat, _packed_of_dense=packed_of_dense, _campos=campos, _cum_tiles=cum)
        global _LAST_INFO
        _LAST_INFO = info
    return rgb, alpha, info


_LAST_INFO = None


def last_info():
    """info dict of the most recent ops.rasterization(want_info=True) call (gsplat's `meta`)."""
    return _LAST_INFO
