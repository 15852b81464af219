"""GPU side of tests/condense_cases.py: csrc/condense.hip through `ops`.  Every focal shape asserts, through
st3r_focal_plan (the function the entry point itself calls), the number of workgroups per view it was built for on a
whole MI355X: a retuned plan fails here instead of thinning the coverage."""
import numpy as np
import pytest
import torch

import condense_cases as cc
from oracle import condense_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    return ops.get_context(torch.device(DEV))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.mark.parametrize("views,H,W,G,why", cc.FOCAL_SHAPES)
def test_focal_shapes(ctx, views, H, W, G, why):
    from starst3r_amd import ops
    assert ops.focal_plan(ctx, views, H, W) == G, why
    canon, pp, _ = cc.focal_views(views, H, W)
    stack = dev(canon)
    fb = ops.focal_weiszfeld_batch(ctx, stack, pp)
    again = ops.focal_weiszfeld_batch(ctx, stack, pp)
    assert torch.equal(fb, again)                                  # the barrier state is rebuilt per call
    got = fb.cpu().numpy().astype(np.float64)
    ref = np.array([co.estimate_focal_knowing_depth(c, pp) for c in canon], np.float64)
    rel = np.abs(got / ref - 1)
    print("focal %d x %dx%d G=%d: worst relative error %.2e (allowed 1e-4)" % (views, H, W, G, rel.max()))
    assert (rel <= 1e-4).all(), (int(rel.argmax()), rel.max())
    single = torch.cat([ops.focal_weiszfeld(ctx, stack[k], pp) for k in range(views)])
    if ops.focal_plan(ctx, 1, H, W) == G:                          # same partials in the same order: same bits
        assert torch.equal(fb, single)
    else:
        np.testing.assert_allclose(got, single.cpu().numpy(), rtol=2e-6)


def test_focal_view_count_limits(ctx):
    from starst3r_amd import ops
    for views in (0, 1025):
        with pytest.raises(ValueError):
            ops.focal_weiszfeld_batch(ctx, torch.ones((views, 8, 8, 3), device=DEV), (4, 4))
        with pytest.raises(ValueError):
            ops.focal_plan(ctx, views, 8, 8)


def test_focal_nan_to_num(ctx):
    from starst3r_amd import ops
    canon, pp, inf_px, nan_px, neg_px = cc.nan_case()
    f = float(ops.focal_weiszfeld(ctx, dev(canon), pp)[0])
    ref = float(co.estimate_focal_knowing_depth(canon, pp))
    assert np.isfinite(f) and abs(f / ref - 1) <= 1e-4, (f, ref)
    base = 16 / (2 * np.tan(np.deg2rad(30)))
    assert 0.5 * base * 1.01 < f < 3.5 * base * 0.99              # not a clipped NaN


@pytest.mark.parametrize("n,H,W,S", cc.CANON_SHAPES)
def test_canonical_view_shapes(ctx, n, H, W, S):
    from starst3r_amd import ops
    X, Cf = cc.canon_case(n, H, W, S)
    canon, canon2, cconf = (t.cpu().numpy() for t in ops.canon_view(ctx, dev(X), dev(Cf), S))
    canon_o, canon2_o, cconf_o = co.canonical_view(X, Cf, S)
    np.testing.assert_allclose(canon, canon_o, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cconf, cconf_o, rtol=1e-5)
    np.testing.assert_allclose(canon2, canon2_o, rtol=1e-4, atol=1e-5)
    assert (canon2[cc.block_centres(H, W, S)] == 1.0).all()       # the closed form at block centres
    if S == 1:
        assert (canon2 == 1.0).all()
    Xe, Ce = cc.canon_case(n, H, W, S, equal_conf=True)
    canon_e, _, cconf_e = (t.cpu().numpy() for t in ops.canon_view(ctx, dev(Xe), dev(Ce), S))
    np.testing.assert_allclose(canon_e, Xe.astype(np.float64).mean(0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cconf_e, 3.0 - 0.999, rtol=1e-5)


@pytest.mark.parametrize("n", cc.ANCHOR_N)
def test_anchor_offsets_truncate(ctx, n):
    from starst3r_amd import ops
    canon2, xy, S = cc.anchor_case(n)
    idx, off = ops.anchor_offsets(ctx, dev(canon2), dev(xy), S)
    idx_o, off_o = co.anchor_depth_offsets(canon2, xy, S)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_o)
    np.testing.assert_allclose(off.cpu().numpy(), off_o, rtol=1e-6)
