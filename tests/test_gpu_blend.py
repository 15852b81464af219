"""Planted-edge parity of the blend kernels (gs_blend.hip, gs_blend_cells.hip, gs_blend_depth.hip) through the C ABI
against oracle/gs_oracle.c, on the hand-written cases of blend_cases.py: list depths 0 .. 769 around the 64 / 256 record
boundaries, equal and unequal neighbours, empty first / middle / last tiles, saturation at every boundary index (all pixels,
a few pixels of one quadrant, none), cell lists of 0 / 1 / 33 / 256 entries and lengths straddling 32 and 64, hard records
(opacity in (0.998, 0.999], clamped opacity 1.2, needle conics) at the first / last / 63rd / 64th position, backward rounds
with 1 .. 64 contributing records per wave, records met by 1 .. 4 waves and spanning 1 .. 6 tiles, slot ranges that cross
a gather window, zero-slot pairs, image sizes 1 / 15 / 16 / 17 modulo 16, one row, one column, 1 x 1.

EVERY pixel counts: the oracle's clear fraction is 1.0 on every case (test_oracle_blend.py), nothing is masked.

Forward bar: rtol 1e-4, atol 1e-5, last_ids equal.  Gradient bounds are not taken from the kernels: per tensor, 4 x the error
the oracle's own float32 pixel arithmetic shows against a float64 evaluation of the same case (blend_cases.grad_bounds),
with 5e-5 of the tensor's maximum as the floor; the element-wise relative error (median, p99) alike with floors 2e-6 / 1e-4.

Template instances reached (st3r_blend_bwd_impl):
  * the stand-alone calls: k_blend_fwd<false>, k_blend_bwd<true> (v_alpha given) and k_blend_bwd<false> (None), slot index
    from reference rectangles; the per-pair sums through k_gather_vtile<9>, those of k_blend_depth_bwd through
    k_gather_vtile<7> (one template, blend_common.h);
  * st3r_gs_raster_train: k_blend_fwd_cells (flag 128: k_blend_fwd<true>) and k_blend_bwd<false> with the packed 10-bit
    `rectbase` (flag 64: `rectbase` NULL, 64-bit packed rectangles).  It never reads debug flag 2 and passes defer == NULL,
    so neither the recomputed tight rectangles nor k_blend_bwd<false, true> (TOUCH) can be reached through it;
  * st3r_gs_train_fwd_bwd (test_train_step_backward_instances_agree, random scenes: it takes Gaussians, not records): flag 2
    (rects == rectbase == NULL, tight = 1: the slot index from recomputed tight rectangles), flag 64, and -- on a scene with
    more than 8 kept records per pair, asserted -- k_blend_bwd<false, true> under flag 0, against the other two
    bit for bit and against the stage path.

Measured on MI355X, worst error / bound per kernel over all cases: MEASURED at the end of this file.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import blend_cases as bc

ALL = list(bc.CASES)


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


_lists = {}


def gpu_lists(ctx, name):
    """records and (record, tile) lists on the GPU, from the pinned bit-exact front-end kernels; equal to the oracle's"""
    if name in _lists:
        return _lists[name]
    from starst3r_amd import ops
    case = bc.get(name)
    tpg, ids_o, flat_o, off_o = case.lists()
    splats = dev(case.records)
    cum, ids, flat = ops.isect(ctx, splats, dev(tpg, torch.int32), case.N, case.Cn, case.W, case.H)
    end_bit = 32 + (case.tw * case.th).bit_length() + case.Cn.bit_length()
    ids_s, flat_s = ops.sort_pairs(ctx, ids, flat, end_bit)
    off = ops.offsets(ctx, ids_s, case.Cn, case.W, case.H)
    torch.cuda.synchronize()
    assert np.array_equal(flat_s.cpu().numpy(), flat_o) and np.array_equal(off.cpu().numpy(), off_o)
    assert np.array_equal(cum.cpu().numpy(), np.cumsum(tpg))
    _lists[name] = (case, splats, off, flat_s, cum)
    return _lists[name]


def forward(ctx, name):
    from starst3r_amd import ops
    case, splats, off, flat, cum = gpu_lists(ctx, name)
    return ops.blend_fwd(ctx, splats, off, flat, case.Cn, case.W, case.H)


def backward(ctx, name, v_rgb, v_alpha):
    """blend_fwd (the hand-off buffers belong to the last forward of the context) then blend_bwd"""
    from starst3r_amd import ops
    case, splats, off, flat, cum = gpu_lists(ctx, name)
    rgb, alpha, last = forward(ctx, name)
    v = ops.blend_bwd(ctx, splats, off, flat, alpha, last, v_rgb, v_alpha, cum, case.Cn, case.W, case.H)
    torch.cuda.synchronize()
    return v


COLS = {"v_means2d": slice(0, 2), "v_opacities": 2, "v_conics": slice(3, 6), "v_colors": slice(6, 9)}


def check_grads(vs, o32, bounds, label, kernel, cols=COLS):
    """vs [Cn * N, 12] against the oracle's per-pair gradients under blend_cases.grad_bounds"""
    assert np.isfinite(vs).all(), label
    for k, col in cols.items():
        b = bounds[k]
        a, ref = vs[:, col], o32[k]
        err = float(np.abs(a - ref).max())
        print("%s %s: max error %.2e = %.3f of the bound (the oracle's own error %.1e; %.1e of the maximum)"
              % (label, k, err, err / b["abs"], b["own"], err / b["scale"]))
        assert err <= b["abs"], (label, k, err, b["abs"])
        if b["big"].sum() >= 50:
            rel = np.abs(a - ref)[b["big"]] / np.abs(ref[b["big"]])
            med, p99 = float(np.median(rel)), float(np.percentile(rel, 99))
            print("    relative error median %.1e (bound %.1e), p99 %.1e (bound %.1e)" % (med, b["med"], p99, b["p99"]))
            assert med <= b["med"] and p99 <= b["p99"], (label, k, med, p99)


def invisible_rows_are_zero(case, vs):
    dead = (case.lists()[0] == 0) | ~(case.opacities > 0)
    assert not vs[dead][:, 0:9].any()
    assert not vs[:, 10:12].any()


# ---- 1. stand-alone forward ----
@pytest.mark.parametrize("name", ALL)
def test_forward_vs_oracle(ctx, name):
    from starst3r_amd import ops
    R = bc.reference(name)["fwd"]
    assert (R["margin"] > 1e-4).all()
    rgb, alpha, last = forward(ctx, name)
    torch.cuda.synchronize()
    np.testing.assert_allclose(rgb.cpu().numpy(), R["rgb"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(alpha.cpu().numpy(), R["alpha"], rtol=1e-4, atol=1e-5)
    assert np.array_equal(last.cpu().numpy(), R["last"])
    # without the per-quadrant relevance test (debug flag 1) every record meets every wave: same images, same indices
    ops.set_debug(ctx, 1)
    try:
        rgb1, alpha1, last1 = forward(ctx, name)
        torch.cuda.synchronize()
    finally:
        ops.set_debug(ctx, 0)
    assert torch.equal(rgb1.view(torch.int32), rgb.view(torch.int32))
    assert torch.equal(alpha1.view(torch.int32), alpha.view(torch.int32)) and torch.equal(last1, last)


# ---- 2. stand-alone backward, both template instances ----
@pytest.mark.parametrize("has_va", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_backward_vs_oracle(ctx, name, has_va):
    R = bc.reference(name)
    case = bc.get(name)
    v_rgb, v_alpha = dev(R["v_rgb"]), (dev(R["v_alpha"]) if has_va else None)
    v = backward(ctx, name, v_rgb, v_alpha)
    again = backward(ctx, name, v_rgb, v_alpha)
    assert torch.equal(v.view(torch.int32), again.view(torch.int32))          # no atomics: bit-reproducible
    vs = v.cpu().numpy()
    B = R["bwd"][has_va]
    check_grads(vs, B["o32"], B["bounds"], "%s v_alpha=%s" % (name, has_va), "k_blend_bwd<%s>" % str(has_va).lower())
    invisible_rows_are_zero(case, vs)
    assert not vs[:, 9].any()


def test_backward_one_hot_cotangents(ctx):
    """a cotangent that is non-zero on one pixel, moved over the four corners of every 4 x 4 cell (which include those of every
    quadrant): the pixel-to-lane mapping of the backward's second phase"""
    name = "onehot16"
    case = bc.get(name); R = bc.reference(name)
    _, _, flat, off = case.lists()
    for cy in range(4):
        for cx in range(4):
            for (ox, oy) in ((0, 0), (3, 0), (0, 3), (3, 3)):
                x, y = 4 * cx + ox, 4 * cy + oy
                v_rgb = np.zeros_like(R["v_rgb"]); v_alpha = np.zeros_like(R["v_alpha"])
                v_rgb[0, y, x] = (1.0, 0.5, -0.25); v_alpha[0, y, x] = 1.0
                o32 = bc.oracle_bwd(case, R["fwd"], v_rgb, v_alpha)
                bounds = bc.grad_bounds(o32, bc.ref64(case, flat, off, v_rgb, v_alpha))
                vs = backward(ctx, name, dev(v_rgb), dev(v_alpha)).cpu().numpy()
                check_grads(vs, o32, bounds, "one-hot (%d, %d)" % (x, y), "k_blend_bwd<true> one-hot")


# ---- 3. depth ----
@pytest.mark.parametrize("name", ALL)
def test_depth_vs_oracle(ctx, name):
    """"uneq" is the case that made k_blend_depth_bwd refine its reciprocal: it ties all depths (z = 1) under a T_final of
    0.09 and a random-sign v_depth, so dL/dalpha = v_d (z T - buf / (1 - alpha)) cancels 11-fold per pixel, the pixel sum
    14-fold again (sum v_d = -15, sum |v_d| = 216), and all 73 records share that one sum.  With the bare v_rcp_f32 (1 ulp,
    carried through the 73-record recurrence T *= 1 / (1 - alpha)) the median relative error of v_means2d was 6.5e-6 against
    a bound of 5.9e-6 (4 x the oracle's own 1.5e-6); with one Newton step on the reciprocal it is 9.4e-7."""
    from starst3r_amd import ops
    case, splats, off, flat, cum = gpu_lists(ctx, name)
    R = bc.reference(name); D = R["depth"]
    rgb, alpha, last = forward(ctx, name)
    d = ops.blend_depth_fwd(ctx, splats, off, flat, alpha, last, case.Cn, case.W, case.H)
    v = ops.blend_depth_bwd(ctx, splats, off, flat, alpha, last, dev(D["v_depth"]), cum, case.Cn, case.W, case.H)
    torch.cuda.synchronize()
    np.testing.assert_allclose(d.cpu().numpy(), D["d"], rtol=1e-4, atol=1e-5 * float(case.depths.max()))
    vs = v.cpu().numpy()
    assert not vs[:, [6, 7, 8, 10, 11]].any()
    o32 = dict(D["o32"]); bounds = dict(D["bounds"])
    o32["v_z"] = o32["v_colors"][:, 0]
    zb = dict(bounds["v_colors"]); zb["big"] = zb["big"][:, 0]; bounds["v_z"] = zb
    cols = {"v_means2d": slice(0, 2), "v_opacities": 2, "v_conics": slice(3, 6), "v_z": 9}
    check_grads(vs, o32, bounds, name + " depth", "k_blend_depth_bwd", cols)
    dead = (case.lists()[0] == 0) | ~(case.opacities > 0)
    assert not vs[dead].any()


# ---- 4. the fused training path ----
# (debug flag 2, "the backward recomputes the rectangles", is read by st3r_gs_train_fwd_bwd only: see
# test_train_step_backward_instances_agree)
FLAGS = {0: "cell-list forward, packed 10-bit rectbase", 128: "quadrant TRAIN forward", 64: "64-bit packed rectangles",
         1: "no quadrant / cell culling"}


@pytest.mark.parametrize("name", bc.FUSED)
def test_fused_raster_train_vs_oracle(ctx, name):
    from starst3r_amd import ops
    case = bc.get(name); F = bc.fused_reference(name)
    rec, gt = dev(case.records), dev(F["gt"])
    n_tiles = case.Cn * case.tw * case.th
    out = {}
    try:
        for flag in FLAGS:
            ops.set_debug(ctx, flag)
            v = torch.full((case.Cn * case.N, 12), float("nan"), device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
            st = ops.raster_train(ctx, rec, case.N, case.Cn, gt, case.W, case.H, 0.2, v, loss)
            torch.cuda.synchronize()
            kept = np.diff(ops.peek(ctx, 1, n_tiles + 1).cpu().numpy()).tolist()
            out[flag] = (v, loss.clone(), st["n_isects"], kept)
    finally:
        ops.set_debug(ctx, 0)
    v0, loss0, n0, kept0 = out[0]
    # exact culling: the records whose alpha >= 1/255 box misses a tile are gone from its list (pinned on the CPU)
    assert kept0 == bc.fused_kept_depths(case) and n0 == sum(kept0)
    assert abs(float(loss0[0]) - F["loss"]) <= 1e-5 * abs(F["loss"]), (float(loss0[0]), F["loss"])
    vs = v0.cpu().numpy()
    check_grads(vs, F["o32"], F["bounds"], name + " fused", "raster_train: k_blend_fwd_cells + k_blend_bwd<false>")
    invisible_rows_are_zero(case, vs)
    for flag, what in FLAGS.items():
        v, loss, n, kept = out[flag]
        assert n == n0 and kept == kept0, what
        assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), what
        assert torch.equal(v.view(torch.int32), v0.view(torch.int32)), what


# ---- 5. relations that cost nothing ----
def test_records_behind_full_saturation_change_nothing(ctx):
    """all records of sat_partial_0 once more behind it: every pixel is saturated when the copies come -- the same image bit
    for bit, no gradient for the copies, the same gradient for the originals"""
    rgb0, alpha0, _ = forward(ctx, "sat_partial_0")
    rgb1, alpha1, _ = forward(ctx, "duplicated")
    torch.cuda.synchronize()
    assert torch.equal(rgb0.view(torch.int32), rgb1.view(torch.int32)) and torch.equal(alpha0, alpha1)
    R = bc.reference("sat_partial_0")
    v_rgb, v_alpha = dev(R["v_rgb"]), dev(R["v_alpha"])                      # same seed, same shape in both cases
    assert np.array_equal(R["v_rgb"], bc.reference("duplicated")["v_rgb"])
    v0 = backward(ctx, "sat_partial_0", v_rgb, v_alpha)
    v1 = backward(ctx, "duplicated", v_rgb, v_alpha)
    n = bc.get("sat_partial_0").N
    assert not bool(v1[n:].any())
    assert torch.equal(v0.view(torch.int32), v1[:n].view(torch.int32))


TRAIN_SCENES = {
    # name: (N, views, W, H, seed, scale_lo, scale_hi, more than 8 kept records per pair?)
    "regular": (400, 3, 96, 64, 7, 0.01, 0.08, False),
    "large": (300, 2, 160, 96, 31, 0.15, 0.3, True),       # Gaussians that cover a third of the 10 x 6 tiles each
}


@pytest.mark.parametrize("which", list(TRAIN_SCENES))
def test_train_step_backward_instances_agree(ctx, which):
    """The backward instances and slot-index forms that only st3r_gs_train_fwd_bwd reaches (deferred gather): packed 10-bit
    `rectbase` (flag 0) -- with k_blend_bwd<false, true> (TOUCH) once a call keeps more than 8 records per pair, which is
    the code's own condition and is asserted for "large" --, 64-bit packed rectangles without `rectbase` (flag 64: never
    TOUCH) and tight rectangles recomputed in the kernel (flag 2: rects == rectbase == NULL).  Same slots, same sums:
    gradients and loss are the same bits under all three, and agree with the reference-exact stage path."""
    from starst3r_amd import ops
    from st3r_synth import synth
    N, V, W, H, seed, lo, hi, touch = TRAIN_SCENES[which]
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=lo, scale_hi=hi)
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, W, H)
    gen = torch.Generator(device=rgb.device).manual_seed(seed)
    gt = torch.clamp(rgb + 0.1 * torch.randn(rgb.shape, device=rgb.device, generator=gen), 0, 1).contiguous()
    sums, v_rgb = ops.loss_l1_ssim(ctx, rgb, gt, 0.8, 0.2)
    v_splats = ops.blend_bwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                             info["_last_ids"], v_rgb, None, info["_cum_tiles"], V, W, H)
    ref = ops.project_sh_bwd(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, campos, W, H,
                             info["_splats"], v_splats, float(V), 0.01, 0.01)
    out = {}
    try:
        for flag in (0, 2, 64):
            ops.set_debug(ctx, flag)
            grads = torch.full((23 * N,), float("nan"), device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
            st = ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, loss)
            torch.cuda.synchronize()
            out[flag] = (grads, loss.clone(), st["n_isects"])
    finally:
        ops.set_debug(ctx, 0)
    g0, l0, n0 = out[0]
    assert (n0 > 8 * N * V) == touch, (n0, N * V)
    assert bool(torch.isfinite(g0).all())
    assert float((g0 - ref).abs().max()) <= 2e-5 * float(ref.abs().max())      # test_fused_train_gradients_equal_stage_path
    for flag in (2, 64):
        gf, lf, nf = out[flag]
        assert nf == n0
        assert torch.equal(lf.view(torch.int32), l0.view(torch.int32)), flag
        assert torch.equal(gf.view(torch.int32), g0.view(torch.int32)), flag


# MEASURED (MI355X), worst error / bound over all cases (the bound: blend_cases.grad_bounds), maximum error | relative
# error distribution (median or p99, whichever is nearer its bound):
#   k_blend_bwd<true>   0.131 | 0.28      k_blend_bwd<false>  0.131 | 0.29      one-hot cotangents  0.014
#   st3r_gs_raster_train (k_blend_fwd_cells + k_blend_bwd<false>)  0.361 | 0.83, bit-identical under flags 128 / 64 / 1
#   k_blend_depth_bwd   0.685 | 0.34  (0.784 before its reciprocal was refined, and 1.10 on the median of "uneq", now 0.16)
#   st3r_gs_train_fwd_bwd, flags 0 (TOUCH on "large") / 2 / 64: the same bits; 2e-5 of the maximum from the stage path
# Run time: 131 cases, 4.5 s alone with start-up.
# Mutations (each run once; all fail here, one of them passes every older blend test): DESIGN.md, "Blend kernels on every
# batch, round, cell and saturation edge".
