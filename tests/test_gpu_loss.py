"""GPU parity tests of the L1 + SSIM loss (csrc/loss.hip) through the C ABI: all three loss kernels -- k_ssim_fwd (value
only), k_ssim_fused<false> (value and gradient) and k_ssim_fused<true> (the same with registered ground-truth moments) --
and k_gt_moments against the float64 oracle, on every launch shape the code distinguishes: no interior, one interior pixel,
every position of the interior's last column relative to a 64-column strip, several row bands (natural and forced), several
views with different content; on uniform noise and on images with the structure of real renders (loss_adam_cases.structured).

The row bands come from loss_bands() in csrc/loss.hip, the one place that holds the rule (a change there is a reason to
revisit the shapes here): per kind of kernel, a number of workgroups to reach or of resident slots to fill, divided by
per_band = ceil(W / 64) * C, and never more than max(1, H // 64) bands.
    ST3R_SSIM_BANDS = n (read on every call) overrides the three loss kernels' count (not k_gt_moments')
    LH = ceil(H / bands) rows per band, ceil(H / LH) bands launched: the last one may be shorter
Every shape below has per_band <= 6, so all four kernels take max(1, H // 64) bands."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as go
import loss_adam_cases as lac

KERNELS = ("k_ssim_fwd", "k_ssim_fused<false>", "k_ssim_fused<true>")

SHAPES = [
    (1, 10, 40), (1, 40, 10),    # no interior: cnt = 0, k_ss = 0
    (1, 11, 11),                 # one interior pixel
    (1, 23, 64),                 # exactly one strip
    (1, 23, 65),                 # a last strip of one column, no interior column in it
    (1, 23, 69),                 # the interior's last column (W - 6 = 63) is a strip's last column
    (1, 23, 70),                 # the interior ends one column past the strip edge
    (2, 12, 75),                 # a last strip (11 columns) narrower than the 20 halo columns staged around it, 2 views
    (1, 130, 70),                # 2 bands of 65 rows, 2 strips
    (2, 141, 139),               # 2 bands of 71 and 70 rows, 3 strips, 2 views
    (1, 257, 75),                # 4 bands of 65, 65, 65 and 62 rows
]
BANDS_SHAPE = (2, 50, 37)
BANDS = (1, 2, 7, 50)            # 7: bands of 8 rows (shorter than the 11-tap window), the last of 2; 50: one-row bands


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def n_bands(H):
    return max(1, H // 64)


def test_band_counts_of_the_shapes_are_what_the_comments_say():
    def rows(H):
        LH = -(-H // n_bands(H))
        return [min(LH, H - i0) for i0 in range(0, H, LH)]
    assert rows(130) == [65, 65] and rows(141) == [71, 70] and rows(257) == [65, 65, 65, 62]
    assert all(len(rows(H)) == 1 for _, H, _ in SHAPES if H < 128)
    assert all(-(-W // 64) * Cn <= 6 for Cn, _, W in SHAPES + [BANDS_SHAPE])   # the per_band term never decides


@functools.lru_cache(maxsize=None)
def case(shape, content):
    """Images [C,H,W,3] (every view its own content: a per-view offset or sum mix-up fails), the oracle's result and the
    gradient bounds per view.  Computed once per (shape, content) and not modified by anyone."""
    Cn, H, W = shape
    xs, ys, refs, bounds = [], [], [], []
    for c in range(Cn):
        seed = 1000 * H + W + 17 * c
        x, y = lac.BUILDERS[content](H, W, seed)
        xs.append(x); ys.append(y)
        refs.append(go.l1_ssim(x, y, lac.W_L1, lac.W_SSIM))
        # Gradient bounds: test_l1_ssim_vs_oracle's (2e-6 of the tensor's maximum, 1e-5 element-wise above 1e-3 of the
        # maximum), measured on noise.  On structured images cancellation makes a plain float32 evaluation of the torch
        # reference ITSELF miss the element-wise bar against float64 (CPU: 2e-5 at 23 x 64 up to 3e-4 at 257 x 75), so there
        # the bound is 4 x that float32 reference's own error on the same image (a different summation order and
        # v_rcp_f32 instead of IEEE division; nothing finer is known), never below the noise bars.
        g_max, g_elem = 2e-6, 1e-5
        if content == "structured":
            e_max, e_elem = lac.float32_reference_error(content, H, W, seed)
            g_max, g_elem = max(g_max, 4 * e_max), max(g_elem, 4 * e_elem)
        bounds.append((g_max, g_elem))
    x, y = np.stack(xs), np.stack(ys)
    x.setflags(write=False); y.setflags(write=False)
    return x, y, refs, bounds


def run_kernels(ctx, X, Y):
    """kernel name -> (sums [C,2] float64, v_render or None) as numpy, plus the moments k_gt_moments wrote."""
    from starst3r_amd import ops
    out = {}
    ops.set_gt_moments(ctx, None, None)
    out[KERNELS[0]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM, want_grad=False)
    out[KERNELS[1]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
    mom = ops.gt_moments(ctx, Y)
    ops.set_gt_moments(ctx, Y, mom)
    try:
        out[KERNELS[2]] = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
        torch.cuda.synchronize()
    finally:
        ops.set_gt_moments(ctx, None, None)
    assert out[KERNELS[0]][1] is None
    return {k: (s.cpu().numpy(), None if v is None else v.cpu().numpy()) for k, (s, v) in out.items()}, mom.cpu().numpy()


def check_against_oracle(tag, kernel, sums, v, shape, refs, bounds):
    """The bounds of test_l1_ssim_vs_oracle per view; prints the worst figures of the launch."""
    Cn, H, W = shape
    cnt = (H - 10) * (W - 10) * 3 if (H > 10 and W > 10) else 0
    worst = dict(l1=0.0, ssim=0.0, gmax=0.0, gelem=0.0)
    fails = []
    for c in range(Cn):
        l1, ss, vr = refs[c]
        e_l1 = abs(sums[c, 0] / (H * W * 3) - l1)
        if cnt:
            e_ss = abs(sums[c, 1] / cnt - ss)
        else:
            e_ss = 0.0
            assert sums[c, 1] == 0.0, (tag, kernel, c, "SSIM sum of an image without interior")
        worst["l1"] = max(worst["l1"], e_l1); worst["ssim"] = max(worst["ssim"], e_ss)
        if e_l1 >= 1e-6: fails.append((c, "mean L1", e_l1, 1e-6))
        if e_ss >= 1e-5: fails.append((c, "mean SSIM", e_ss, 1e-5))
        if v is not None:
            assert np.isfinite(v[c]).all(), (tag, kernel, c)
            g_max, g_elem = lac.grad_errors(v[c], vr)
            worst["gmax"] = max(worst["gmax"], g_max); worst["gelem"] = max(worst["gelem"], g_elem)
            if g_max > bounds[c][0]: fails.append((c, "gradient of max", g_max, bounds[c][0]))
            if g_elem > bounds[c][1]: fails.append((c, "gradient element-wise", g_elem, bounds[c][1]))
    b = (max(b[0] for b in bounds), max(b[1] for b in bounds))
    print(f"LOSS {tag} {kernel}: L1 {worst['l1']:.2e} (1e-6) SSIM {worst['ssim']:.2e} (1e-5)"
          + ("" if v is None else f" grad/max {worst['gmax']:.2e} ({b[0]:.2e}) grad/elem {worst['gelem']:.2e} ({b[1]:.2e})"))
    assert not fails, (tag, kernel, fails)


@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_kernels_vs_oracle(ctx, shape, content):
    Cn, H, W = shape
    x, y, refs, bounds = case(shape, content)
    res, _ = run_kernels(ctx, dev(x), dev(y))
    tag = f"{Cn}x{H}x{W} {content}"
    for kernel in KERNELS:
        check_against_oracle(tag, kernel, *res[kernel], shape, refs, bounds)
    # the two fused kernels take the ground truth's taps in the same order: same gradient bits
    assert np.array_equal(res[KERNELS[1]][1].view(np.int32), res[KERNELS[2]][1].view(np.int32))
    if H < 11 or W < 11:
        # no interior: k_ss = 0 and every derivative map is zero, so the gradient is EXACTLY the L1 term, k_l1 formed as
        # st3r_loss_impl forms it -- float(double(float w_l1) / (H W 3)) -- times sign(x - y)
        k_l1 = np.float32(np.float64(np.float32(lac.W_L1)) / (H * W * 3))
        want = k_l1 * np.sign(x - y).astype(np.float32)
        assert want.dtype == np.float32 and (np.sign(x - y) == 0).any() == (content == "structured")
        for kernel in KERNELS[1:]:
            assert np.array_equal(res[kernel][1], want), kernel


@pytest.mark.parametrize("shape", SHAPES + [BANDS_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_gt_moments_vs_float64_convolution(ctx, shape):
    """k_gt_moments on every shape (its band rule is k_ssim_fwd's; the forcing hook does not reach it): the interior within
    2e-6 of a float64 separable convolution of y and y^2 (the bar of test_gt_moments_change_no_bit_of_the_loss), everything
    else exactly zero -- all of it where the image has no interior."""
    from starst3r_amd import ops
    Cn, H, W = shape
    for content in sorted(lac.BUILDERS):
        _, y, _, _ = case(shape, content)
        M = ops.gt_moments(ctx, dev(y))
        torch.cuda.synchronize()
        M = M.cpu().numpy().astype(np.float64)
        assert M.shape == (Cn, H, W, 3, 2)
        border = np.ones((H, W), bool)
        if H > 10 and W > 10:
            border[5:H - 5, 5:W - 5] = False
            yd = y.astype(np.float64)
            e0 = np.abs(M[:, 5:H - 5, 5:W - 5, :, 0] - lac.conv_valid(yd)).max()
            e1 = np.abs(M[:, 5:H - 5, 5:W - 5, :, 1] - lac.conv_valid(yd * yd)).max()
            print(f"LOSS {Cn}x{H}x{W} {content} k_gt_moments: conv(y) {e0:.2e} conv(y^2) {e1:.2e} (2e-6)")
            assert e0 < 2e-6 and e1 < 2e-6
        assert border.any() and np.all(M[:, border] == 0.0)


@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
def test_forced_row_bands(ctx, monkeypatch, content):
    """ST3R_SSIM_BANDS on 2 x 50 x 37: 1, 2, 7 (bands of 8 rows, shorter than the window; a last band of 2) and 50 (one-row
    bands).  Every setting meets the oracle in all three kernels.  Which band a pixel falls in changes neither its taps nor
    their order -- a band recomputes its halo rows, it does not take them from its neighbour -- so v_render is the same BITS
    under all four settings.  The sums are not: a workgroup adds its band's rows up in float32 before the double-precision
    atomic, so another band height groups the float32 additions differently (what the oracle bars above already hold);
    at ONE setting the two fused kernels group alike and agree to the order of the double atomics, rtol 1e-13 like
    test_gt_moments_change_no_bit_of_the_loss."""
    Cn, H, W = BANDS_SHAPE
    x, y, refs, bounds = case(BANDS_SHAPE, content)
    X, Y = dev(x), dev(y)
    res = {}
    for nb in BANDS:
        monkeypatch.setenv("ST3R_SSIM_BANDS", str(nb))
        res[nb], _ = run_kernels(ctx, X, Y)
    monkeypatch.delenv("ST3R_SSIM_BANDS")
    for nb in BANDS:
        for kernel in KERNELS:
            check_against_oracle(f"{Cn}x{H}x{W} {content} bands={nb}", kernel, *res[nb][kernel], BANDS_SHAPE, refs, bounds)
        np.testing.assert_allclose(res[nb][KERNELS[2]][0], res[nb][KERNELS[1]][0], rtol=1e-13, atol=0)
    for kernel in KERNELS[1:]:
        same = [np.array_equal(res[nb][kernel][1].view(np.int32), res[1][kernel][1].view(np.int32)) for nb in BANDS]
        spread = max(np.abs(res[nb][kernel][0] / res[1][kernel][0] - 1).max() for nb in BANDS)
        print(f"LOSS bands {content} {kernel}: v_render bit-identical to 1 band at {dict(zip(BANDS, same))}, "
              f"sums differ by at most {spread:.2e} (relative)")
        assert all(same), (kernel, dict(zip(BANDS, same)))


def test_registered_moments_are_what_the_fused_kernel_reads(ctx):
    """The comparisons above say nothing about k_ssim_fused<true> if the registration silently misses and
    k_ssim_fused<false> runs in its place: with WRONG moments registered the result must change."""
    from starst3r_amd import ops
    x, y, _, _ = case((1, 23, 70), "noise")
    X, Y = dev(x), dev(y)
    _, v0 = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
    wrong = torch.zeros((*Y.shape, 2), device="cuda:0")
    ops.set_gt_moments(ctx, Y, wrong)
    try:
        _, v1 = ops.loss_l1_ssim(ctx, X, Y, lac.W_L1, lac.W_SSIM)
        torch.cuda.synchronize()
    finally:
        ops.set_gt_moments(ctx, None, None)
    assert not torch.equal(v0, v1)
