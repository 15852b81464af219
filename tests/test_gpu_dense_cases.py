"""GPU side of tests/dense_cases.py: csrc/dense.hip through `ops`.  Every point of every case is compared; the cleaned
confidences for equal bits."""
import numpy as np
import pytest
import torch

import dense_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    return ops.get_context(torch.device(DEV))


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def unproject(ctx, c):
    from starst3r_amd import ops
    pts, z = ops.dense_unproject(ctx, t(c["start"], torch.int32), t(c["pix"]), t(c["idx"], torch.int32), t(c["off"]),
                                 t(c["core"]), t(c["cam"]), t(c["base_f"]))
    return pts, z


def clean(ctx, c, pts, z, conf, tol, bad_conf):
    from starst3r_amd import ops
    return ops.dense_clean(ctx, t(c["start"], torch.int32), t(np.array(c["sizes"]), torch.int32), t(c["cam"]), t(pts),
                           t(z), t(conf), tol=tol, bad_conf=bad_conf).cpu().numpy()


@pytest.mark.parametrize("name", ["c3", "c4", "c1"])
def test_mixed_sizes(ctx, name):
    c = dc.mixed_case(name)
    pts, z = unproject(ctx, c)
    pts, z = pts.cpu().numpy(), z.cpu().numpy()
    pts_ref, z_ref = dc.unproject_ref(c)
    np.testing.assert_allclose(pts, pts_ref, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(z, z_ref, rtol=1e-5)
    for k in range(c["C"]):                                      # view_of at every view's first and last pixel
        for e in (c["start"][k], c["start"][k + 1] - 1):
            np.testing.assert_allclose(pts[e], pts_ref[e], rtol=2e-5, atol=2e-5)
    got = clean(ctx, c, pts, z, c["conf"], 0.001, 0.0)
    if c["C"] == 1:
        np.testing.assert_array_equal(got, c["conf"])            # nobody to be compared with
        return
    margin = []
    want = dc.clean_oracle(c, c["conf"], pts, z, 0.001, 0.0, margin=margin)   # the kernel's own float32 points
    assert np.concatenate(margin).min() > 2e-3
    np.testing.assert_array_equal(got, want.astype(F))           # every point


@pytest.mark.parametrize("C", [64, 512])
def test_many_views(ctx, C):
    c = dc.many_views_case(C)
    pts, z = unproject(ctx, c)
    pts_ref, z_ref = dc.unproject_ref(c)
    np.testing.assert_array_equal(pts.cpu().numpy(), pts_ref.astype(F))     # dyadic inputs: exact
    np.testing.assert_array_equal(z.cpu().numpy(), z_ref.astype(F))
    got = clean(ctx, c, pts_ref, z_ref, c["conf"], 0.001, 0.0)
    np.testing.assert_array_equal(got, dc.clean_vectorised(c, c["conf"], pts_ref, z_ref, 0.001, 0.0).astype(F))


def test_view_count_limit(ctx):
    c = dc.many_views_case(513)
    with pytest.raises(ValueError):
        clean(ctx, c, np.zeros((16 * 513, 3), F), np.ones(16 * 513, F), c["conf"], 0.001, 0.0)


@pytest.mark.parametrize("bad_conf", [0.0, 0.5, 9.0])
def test_planted_decisions(ctx, bad_conf):
    c = dc.planted_case()
    got = clean(ctx, c, c["pts"], c["zcam"], c["conf"], c["tol"], bad_conf)
    want = dc.clean_oracle(c, c["conf"], c["pts"], c["zcam"], c["tol"], bad_conf).astype(F)
    wrong = np.nonzero(got != want)[0]
    assert len(wrong) == 0, [(int(k), c["what"][k] if k < len(c["what"]) else "target", float(got[k]), float(want[k])) for k in wrong]


def test_update_order(ctx):
    c = dc.order_case()
    got = clean(ctx, c, c["pts"], c["zcam"], c["conf"], c["tol"], c["bad_conf"])
    assert got.tolist() == [1.0, 1.0, 0.5, 2.0, 5.0, 1.0], got.tolist()
