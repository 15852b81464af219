"""CPU pins of tests/condense_cases.py with oracle/condense_oracle.py alone (no GPU): every focal shape has the
workgroup layout it names under the plan's arithmetic, the nan_to_num pixels are there and matter, the canonical-view
shapes cover the block sizes they name and have canon2 == 1 at every block centre, and the anchor pixels carry every
fraction and border they claim."""
import numpy as np
import pytest

import condense_cases as cc
from oracle import condense_oracle as co

F = np.float32


def test_focal_shapes_are_what_they_name():
    """`plan_G` lays the shapes out without a GPU; that it IS the library's plan is asserted on the GPU, case by case,
    through st3r_focal_plan."""
    for views, H, W, G, _why in cc.FOCAL_SHAPES:
        assert cc.plan_G(views, H, W) == G and G * views <= 1024
        sizes = [cc.pixels_of_workgroup(H, W, G, g) for g in range(G)]
        assert sum(sizes) == H * W and min(sizes) > 0
    assert cc.pixels_of_workgroup(15, 17, 1, 0) == 255
    assert cc.pixels_of_workgroup(1, 257, 2, 1) == 1
    assert cc.pixels_of_workgroup(40, 48, 8, 7) == 128
    assert 12 & 11 and 3 * 300 == 900
    # half the device's workgroups bound the grid: a smaller device thins G instead of hanging
    assert cc.plan_G(17, 48, 64, resident=100) == 5 and cc.plan_G(300, 24, 32, resident=100) == 1


@pytest.mark.parametrize("views,H,W", [(s[0], s[1], s[2]) for s in cc.FOCAL_SHAPES if s[0] <= 17])
def test_focal_inputs_are_inside_the_clip_range_and_the_outliers_matter(views, H, W):
    canon, pp, f_true = cc.focal_views(views, H, W)
    base = max(H, W) / (2 * np.tan(np.deg2rad(30)))
    assert canon.shape == (views, H, W, 3) and (canon[..., 2] > 1).all()
    got = np.array([co.estimate_focal_knowing_depth(c, pp) for c in canon], np.float64)
    assert (got > 0.5 * base * 1.02).all() and (got < 3.5 * base * 0.98).all()
    if H > 1:
        assert len(np.unique(np.round(got, 3))) == views
    # the L2 start (no re-weighting) differs: the Weiszfeld passes are being exercised
    l2 = np.array([cc.focal_no_nan_to_num(c, pp) for c in canon], np.float64)
    assert (np.abs(l2 / got - 1) > 1e-3).any()


def test_nan_case():
    canon, pp, inf_px, nan_px, neg_px = cc.nan_case()
    c = canon.reshape(-1, 3)
    assert len(inf_px) == len(nan_px) == len(neg_px) == 5 and len(set(inf_px) | set(nan_px) | set(neg_px)) == 15
    with np.errstate(all="ignore"):
        q = c[:, :2] / c[:, 2:3]
    assert np.isinf(q[inf_px]).any(1).all() and np.isnan(q[nan_px]).all() and (c[neg_px, 2] < 0).all()
    assert np.isfinite(np.delete(q, np.concatenate([inf_px, nan_px]), 0)).all()
    f = co.estimate_focal_knowing_depth(canon, pp)
    base = 16 / (2 * np.tan(np.deg2rad(30)))
    assert np.isfinite(f) and 0.5 * base < f < 3.5 * base
    # without the branch the very first pass is NaN: it matters
    assert np.isnan(cc.focal_no_nan_to_num(canon, pp))
    # a z == 0 pixel that went through nan_to_num adds 0 to both sums: it equals a removed pixel by construction, so
    # "removed" can only differ through the z < 0 pixels -- which do count, with the sign of x / z flipped
    gone = canon.copy().reshape(-1, 3); gone[neg_px] = 0
    assert co.estimate_focal_knowing_depth(gone.reshape(16, 16, 3), pp) != f


@pytest.mark.parametrize("n,H,W,S", cc.CANON_SHAPES)
def test_canon_case(n, H, W, S):
    X, Cf = cc.canon_case(n, H, W, S)
    assert H % S == 0 and W % S == 0 and (X[..., 2] > 0.5).all() and (Cf > 1).all()
    canon, canon2, cconf = co.canonical_view(X, Cf, S)
    ctr = cc.block_centres(H, W, S)
    assert (canon2[ctr] == 1.0).all()              # r = 1e-8, angle 0: exactly 1 at block centres, for every n
    if S == 1:
        assert (canon2 == 1.0).all()
    else:
        assert (canon2 != 1.0).sum() >= H * W - (H // S) * (W // S) - 2
    Xe, Ce = cc.canon_case(n, H, W, S, equal_conf=True)
    canon_e, _, cconf_e = co.canonical_view(Xe, Ce, S)
    np.testing.assert_allclose(canon_e, Xe.astype(np.float64).mean(0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cconf_e, 3.0 - 0.999, rtol=1e-5)


def test_canon_shapes_cover_what_they_name():
    S = {s[3] for s in cc.CANON_SHAPES}; n = {s[0] for s in cc.CANON_SHAPES}; hw = {s[1] * s[2] for s in cc.CANON_SHAPES}
    assert {1, 2, 8} <= S and n == {1, 2, 12} and {255, 256, 320} <= hw
    assert any(s[1] == s[2] == s[3] for s in cc.CANON_SHAPES)


@pytest.mark.parametrize("n", cc.ANCHOR_N)
def test_anchor_case(n):
    canon2, xy, S = cc.anchor_case(n)
    H, W = canon2.shape
    assert (xy >= 0).all() and (xy[:, 0] < W).all() and (xy[:, 1] < H).all()
    assert xy[-1, 0] == np.nextafter(F(W), F(0)) and xy[-1, 1] == np.nextafter(F(H), F(0))
    idx, off = co.anchor_depth_offsets(canon2, xy, S)
    assert idx.min() >= 0 and idx.max() < (H // S) * (W // S) and idx[-1] == (H // S) * (W // S) - 1
    if n >= 255:
        fr = np.rint((xy.astype(np.float64) - np.floor(xy)) * 1000).astype(int)
        assert {0, 490, 500, 999} <= set(fr[:, 0].tolist()) and {0, 490, 500, 999} <= set(fr[:, 1].tolist())
        bx, by = np.floor(xy[:, 0]) // S, np.floor(xy[:, 1]) // S
        assert {0, W // S - 1} <= set(bx) and {0, H // S - 1} <= set(by)
        # rounding instead of truncating would move pixels (and leave the image at the far borders)
        moved = (np.rint(xy) != np.floor(xy)).any(1)
        assert moved.sum() > n // 4 and (np.rint(xy[:, 0]) >= W).any()
