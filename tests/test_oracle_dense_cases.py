"""CPU pins of tests/dense_cases.py with oracle/dense_oracle.py alone (no GPU): the mixed-size inputs clear the
oracle's decision margin on every point, each planted point does what its label says, the order case really depends
on the order, and the vectorised reference used for many views is the oracle's function."""
import numpy as np
import pytest

import dense_cases as dc

F = np.float32


@pytest.mark.parametrize("name", ["c3", "c4", "c1"])
def test_mixed_sizes_all_points_clear(name):
    c = dc.mixed_case(name)
    sizes = c["sizes"]
    assert len({s for s in sizes}) == len(sizes)                        # no two views of one size
    if name == "c3":
        assert sizes == [(5, 7), (16, 16), (3, 40)] and sizes[-1][0] * sizes[-1][1] < 256   # the last view is not the largest
    if name == "c4":
        assert sizes[1] == (1, 1)
    assert c["start"].tolist() == np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).tolist()
    assert len(np.unique(c["cam"][:, 12])) == c["C"] and len(np.unique(c["base_f"])) == c["C"]
    pts, z = dc.unproject_ref(c)
    assert (z > 0.5).all()
    # a pixel unprojected with a neighbouring view's row is somewhere else: view_of errors show at every view edge
    for k in range(1, c["C"]):
        assert (np.abs(c["cam"][k, 9:17] - c["cam"][k - 1, 9:17]) > 1e-2).all()   # T, f, cx, cy, A, B all differ
    if c["C"] == 1:
        return
    margin = []
    want = dc.clean_oracle(c, c["conf"], pts.astype(F), z.astype(F), 0.001, 0.0, margin=margin)
    margin = np.concatenate(margin)
    assert margin.min() > 2e-3, margin.min()                           # EVERY point: nothing needs masking
    lowered = want < c["conf"]
    assert lowered.sum() >= 5, lowered.sum()
    np.testing.assert_array_equal(dc.clean_vectorised(c, c["conf"], pts.astype(F), z.astype(F), 0.001, 0.0), want)


@pytest.mark.parametrize("C", [64, 512])
def test_many_views_are_exact(C):
    c = dc.many_views_case(C)
    pts, z = dc.unproject_ref(c)
    assert (pts.astype(F) == pts).all() and (z.astype(F) == z).all() and set(np.unique(z)) == {2.0, 4.0}
    want = dc.clean_vectorised(c, c["conf"], pts, z, 0.001, 0.0)
    assert 0.05 < (want < c["conf"]).mean() < 0.6
    if C == 64:
        np.testing.assert_array_equal(dc.clean_oracle(c, c["conf"], pts, z, 0.001, 0.0), want)


def test_planted_points_do_what_they_say():
    c = dc.planted_case()
    n0 = c["sizes"][0][1]
    assert len(c["what"]) == n0 == 34
    for bad_conf in (0.0, 0.5, 9.0):
        want = dc.clean_oracle(c, c["conf"], c["pts"], c["zcam"], c["tol"], bad_conf)
        np.testing.assert_array_equal(dc.clean_vectorised(c, c["conf"], c["pts"], c["zcam"], c["tol"], bad_conf), want)
        np.testing.assert_array_equal(want[n0:], c["conf"][n0:])        # the targets' own points are never touched
        for k, what in enumerate(c["what"]):
            lowered = want[k] < c["conf"][k]
            if bad_conf == 9.0:
                assert not lowered, what                                # above every confidence: unchanged
            elif "(lowered)" in what or "lowered)" in what:
                assert lowered and want[k] == min(c["conf"][k], bad_conf), what
            elif "kept at 0.25" in what:
                assert lowered == (bad_conf == 0.0), what
            else:
                assert "kept" in what and not lowered, what
    # every projection is exact: float32 evaluation of u for the tie points
    P = c["pts"][:n0]
    for T, tag in ((np.zeros(3, F), "t1"), (np.array([16, 0, 0], F), "t2")):
        sel = [k for k, w in enumerate(c["what"]) if w.startswith(tag) and "u=2.5 ->" in w]
        for k in sel:
            d = P[k] - T
            assert (F(2) * d[0] + F(0.5) * d[2]) / d[2] == F(2.5)


def test_order_case_depends_on_the_order():
    c = dc.order_case()
    want = dc.clean_oracle(c, c["conf"], c["pts"], c["zcam"], c["tol"], c["bad_conf"])
    assert want.tolist() == [1.0, 1.0, 0.5, 2.0, 5.0, 1.0]            # P0 lowered, Q1 kept
    rev = dc.clean_oracle(c, c["conf"], c["pts"], c["zcam"], c["tol"], c["bad_conf"], order=[2, 1, 0])
    assert rev.tolist() == [1.0, 1.0, 0.5, 0.5, 5.0, 1.0]             # reverse order: Q1 lowered as well
    snap = dc.clean_vectorised(c, c["conf"], c["pts"], c["zcam"], c["tol"], c["bad_conf"], snapshot=True)
    assert snap.tolist() == rev.tolist()                               # uncleaned confidences: the same wrong answer
    np.testing.assert_array_equal(dc.clean_vectorised(c, c["conf"], c["pts"], c["zcam"], c["tol"], c["bad_conf"]), want)
