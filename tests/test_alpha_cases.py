"""CPU-only: the float64 references of tests/alpha_cases.py against torch autograd in float64, and the promise their inputs
make -- that float32 evaluates every formula of the background / alpha kernels exactly, so the GPU tests may ask for bits."""
import numpy as np
import pytest
import torch

import alpha_cases as ac
from per_view_kernel_cases import STREAM_SHAPES

SHAPES = [s for s in STREAM_SHAPES if s[0] * s[1] * s[2] <= 300000]   # (the largest stream shape adds nothing on the CPU)


def _ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_the_inputs_are_what_the_docstring_says(shape):
    C, H, W = shape
    d = ac.inputs(shape)
    assert set(np.unique(d["alpha"])) <= set(ac.ALPHAS.tolist())
    for k, unit, lo, hi in (("x", 16, 0, 1), ("b", 16, 0, 1), ("v", 8, -2, 2), ("v_in", 8, -2, 2)):
        a = d[k].astype(np.float64)
        assert np.array_equal(a * unit, np.round(a * unit)) and a.min() >= lo and a.max() <= hi, k
    on, w, M = d["on"], d["w"], d["M"]
    assert np.array_equal(on, w > 0)
    assert not np.isfinite(M[~on]).any() and np.isfinite(M[on]).all()
    assert np.array_equal(M[on] * 16, np.round(M[on] * 16)) and M[on].min() >= 0 and M[on].max() <= 1
    if H * W >= 500:
        assert (w == 0).any() and (w < 0).any() and np.isnan(w).any() and np.isnan(M).any() and np.isinf(M).any()
    a = d["alpha"][..., 0]
    assert np.array_equal(a[d["tie"]], M[d["tie"]])
    if C > 1:
        assert not on[C - 1].any()                                   # a view without weight
        assert on[0].any() and np.array_equal(a[0][on[0]], M[0][on[0]])   # a view with a == M wherever it counts


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_references_agree_with_torch_autograd_in_float64(shape):
    d = ac.inputs(shape)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    x, a, b, v = t(d["x"]), t(d["alpha"]).requires_grad_(), t(d["b"]).requires_grad_(), t(d["v"])
    y = x + (1 - a) * b[:, None, None, :]
    assert np.abs(y.detach().numpy() - ac.composite_reference(d["x"], d["alpha"], d["b"])).max() <= 1e-12
    (y * v).sum().backward()
    ref = ac.alpha_grad_reference(d["alpha"], d["b"], d["v"], rounded=False)
    assert np.array_equal(a.grad.numpy()[..., 0], ref["t_bg"])       # dyadic: exact in any association
    assert np.abs(b.grad.numpy() - ref["v_b"]).max() <= 1e-12 * max(1.0, np.abs(ref["v_b"]).max())
    # the alpha term: weights that do not count are dropped before the formula (a NaN times zero is a NaN)
    on = d["on"]
    w = t(np.where(on, d["w"], 0.0)); M = t(np.where(on, d["M"], 0.0))
    a2 = t(d["alpha"]).requires_grad_()
    n_c = torch.clamp(w.sum((1, 2)), min=1.0)
    per_view = (w * (a2[..., 0] - M).abs()).sum((1, 2))
    loss = (ac.ALPHA_FAC * per_view / n_c).sum()
    loss.backward()
    ref = ac.alpha_grad_reference(d["alpha"], None, None, d["M"], d["w"], rounded=False)
    assert np.array_equal(n_c.numpy(), ref["n_c"]) and np.array_equal(per_view.detach().numpy(), ref["sums"])
    loss = float(loss.detach())
    assert abs(loss - float((ac.ALPHA_FAC * ref["sums"] / ref["n_c"]).sum())) <= 1e-12 * max(1.0, abs(loss))
    g = a2.grad.numpy()[..., 0]
    decided = on & ~d["tie"] & (ref["diff"] != 0)
    assert np.array_equal(np.sign(g), np.sign(ref["t_a"]))           # the sign, 0 on ties and without weight
    assert np.all(g[~decided] == 0) and np.all(ref["t_a"][~decided] == 0)     # exactly equal where there is no sign
    # Where the sign is decided the gradient is +- alpha_fac w / n_c.  The reference rounds alpha_fac / n_c, then the product
    # with w; torch associates as it likes (observed: equal bits on five of these shapes, 1 ulp off on 8x120x160 and
    # 256x4x4), so equal bits cannot be asked of the loss as written here.  Both are two roundings away from the real number,
    # each within 2^-53 relative: per element they differ by at most 4 * 2^-53 |t_a| <= 2 spacing(|t_a|).
    err = np.abs(g - ref["t_a"])[decided] / np.spacing(np.abs(ref["t_a"][decided]))
    print(_ids(shape), "alpha term, torch against the reference: at worst %.1f ulp" % (err.max() if err.size else 0.0))
    assert np.all(err <= 2.0)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_float32_evaluates_every_formula_exactly(shape):
    d = ac.inputs(shape)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    # the composite: float32 arithmetic, fused or not, gives the float64 value
    y64 = ac.composite_reference(d["x"], d["alpha"], d["b"])
    y32 = ac.composite_reference(d["x"], d["alpha"], d["b"], np.float32)
    assert y32.dtype == np.float32 and np.array_equal(y32.view(np.int32), f32(y64).view(np.int32))
    assert np.array_equal(f32(y64).astype(np.float64), y64)          # nothing was rounded at all
    for bg in (False, True):
        for at in (False, True):
            if not (bg or at):
                continue
            for acc in (False, True):
                kw = dict(b=d["b"] if bg else None, v=d["v"] if bg else None, M=d["M"] if at else None,
                          w=d["w"] if at else None, v_in=d["v_in"] if acc else None)
                ref = ac.alpha_grad_reference(d["alpha"], **kw)
                got = ac.alpha_grad_float32(d["alpha"], **kw)
                assert np.array_equal(got.view(np.int32), f32(ref["v_alpha"]).view(np.int32)), (bg, at, acc)
                if bg:      # t_bg and the sums lose nothing in float32 / double
                    assert np.array_equal(f32(ref["t_bg"]).astype(np.float64), ref["t_bg"])
                    terms = (1.0 - d["alpha"].astype(np.float64)) * d["v"].astype(np.float64)
                    assert np.array_equal(terms * 32, np.round(terms * 32)) and np.abs(terms).sum() < 2.0 ** 45
                if at:
                    assert np.array_equal(ref["terms"] * 128, np.round(ref["terms"] * 128)) and ref["terms"].sum() < 2.0 ** 45
                    assert np.array_equal(ref["sums"] * 128, np.round(ref["sums"] * 128))


def test_zero_weight_pixels_and_views_get_exact_zeros():
    d = ac.inputs((3, 33, 32))
    ref = ac.alpha_grad_reference(d["alpha"], None, None, d["M"], d["w"])
    assert np.all(ref["t_a"][~d["on"]] == 0) and np.isfinite(ref["v_alpha"]).all()
    assert ref["n_c"][-1] == 1.0 and ref["sums"][-1] == 0.0 and np.all(ref["v_alpha"][-1] == 0)
    assert ref["n_c"][0] > 1.0 and ref["sums"][0] == 0.0 and np.all(ref["v_alpha"][0] == 0)   # a == M everywhere
    assert ref["sums"][1] > 0 and np.abs(ref["v_alpha"][1]).max() > 0
