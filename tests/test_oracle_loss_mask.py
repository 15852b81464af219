"""CPU-only: the float64 reference of the weighted L1 + SSIM loss (tests/loss_mask_cases.py) against the reference the
unweighted loss tests use, against central differences, and on a view without weight."""
import numpy as np
import pytest
import torch

import loss_adam_cases as lac
import loss_mask_cases as lmc


@pytest.mark.parametrize("content", sorted(lac.BUILDERS))
@pytest.mark.parametrize("shape", [(23, 70), (14, 13), (10, 40)], ids=lambda s: "x".join(map(str, s)))
def test_all_ones_reproduce_the_unweighted_reference(shape, content):
    H, W = shape
    x, y = lac.BUILDERS[content](H, W, 1000 * H + W)
    l1, ss, grad = lac.torch_loss_grad(x, y, torch.float64)
    r = lmc.weighted_loss_grad(x, y, lmc.w_ones(H, W, 0))
    has_interior = H > 10 and W > 10
    assert r["n1"] == H * W and r["n2"] == ((H - 10) * (W - 10) if has_interior else 1)
    assert abs(r["l1"] - l1) < 1e-12 and abs(r["ssim"] - ss) < 1e-12
    if has_interior:
        assert abs(r["loss"] - (lac.W_L1 * l1 + lac.W_SSIM * (1 - ss))) < 1e-12
        assert np.abs(r["grad"] - grad).max() < 1e-12
    else:   # section 1 of the weighted loss: an empty interior contributes 0 (the unweighted loss counts 1 - 0 there)
        assert abs(r["loss"] - lac.W_L1 * l1) < 1e-12
        assert np.abs(r["grad"] - grad).max() < 1e-12   # (the SSIM term has no gradient either way)


@pytest.mark.parametrize("builder", ["uniform", "holes", "interior_only", "border_pixel"])
def test_gradient_matches_central_differences(builder):
    H, W = 14, 13
    x, y = lac.noise(H, W, 5)
    w = lmc.weights_for(builder, 1, H, W, 9)[0]
    r = lmc.weighted_loss_grad(x, y, w)
    xd = x.astype(np.float64)
    rng = np.random.default_rng(0)
    picks = [(int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(3))) for _ in range(40)]
    picks += [(i, j, 0) for i, j in zip(*np.nonzero(w)) if not (5 <= i < H - 5 and 5 <= j < W - 5)][:4]
    h = 1e-6
    worst = 0.0
    for i, j, ch in picks:
        if abs(xd[i, j, ch] - y[i, j, ch]) < 10 * h:   # the kink of |gt - r|
            continue
        xp, xm = xd.copy(), xd.copy()
        xp[i, j, ch] += h; xm[i, j, ch] -= h
        fd = (lmc.weighted_loss_grad(xp, y, w)["loss"] - lmc.weighted_loss_grad(xm, y, w)["loss"]) / (2 * h)
        worst = max(worst, abs(fd - r["grad"][i, j, ch]))
    scale = np.abs(r["grad"]).max()
    print(f"central differences, {builder}: worst {worst:.2e} against a largest entry of {scale:.2e}")
    # float64 differences of a loss of order 1 with h = 1e-6: rounding 1e-16 / 1e-6 = 1e-10, truncation h^2 f''' smaller
    assert scale > 0 and worst < 1e-8


def test_a_view_without_weight_gives_zero_loss_and_zero_gradient():
    H, W = 23, 30
    x, y = lac.structured(H, W, 3)
    r = lmc.weighted_loss_grad(x, y, lmc.w_zero(H, W, 0))
    assert r["loss"] == 0.0 and r["l1"] == 0.0 and r["ssim"] == 0.0 and r["n1"] == 1.0 and r["n2"] == 1.0
    assert np.all(r["grad"] == 0.0)
    maps = lmc.weights_for("zero_view", 3, H, W, 4)
    assert np.all(maps[-1] == 0.0) and maps[0].max() > 1.0 and maps[1].min() >= 0.0


def test_the_builders_are_what_their_names_say():
    H, W = 23, 70
    interior = np.zeros((H, W), bool); interior[5:H - 5, 5:W - 5] = True
    w = lmc.w_border_pixel(H, W, 0)
    assert np.count_nonzero(w) == 1 and not interior[w > 0].any()
    w = lmc.w_interior_only(H, W, 0)
    assert np.all(w[~interior] == 0) and np.all(w[interior] > 0)
    w = lmc.w_holes(H, W, 0)
    assert set(np.unique(w)) == {0.0, 1.0} and 0.2 < (w == 0).mean() < 0.8
    w = lmc.w_uniform(H, W, 0)
    assert w.min() >= 0 and 1.5 < w.max() <= 2.0
    assert np.all(lmc.w_interior_only(10, 40, 0) == 0) and np.count_nonzero(lmc.w_border_pixel(10, 40, 0)) == 1
