"""CPU pins of tests/align_cases.py -- the inputs of test_gpu_align_cases.py -- with oracle/align_oracle.py alone (no GPU):
every case has the launch shape, the tree, the ties and the clamp rows it names (counted from the float64 oracle's own
values, asserted, not assumed); the host formulas for rows per workgroup, partials and LDS bytes that the cases are laid
out by are the ones in align.hip, on both sides of each threshold; no row of any case sits near a branch threshold, where
float32 and float64 may take different sides; and no bound -- 4 x the float32 oracle's own error, floored -- exceeds the
2e-3 the older gradient checks allow, except in the one case that says so (`clamp_behind_s2`).
"""
import os
import re

import numpy as np
import pytest
import torch

import align_cases as ac

ALL = list(ac.CASES)
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "starst3r_amd", "csrc", "align.hip")


def test_host_formulas_are_those_of_the_library():
    """`launch_shape` / `lds_bytes` restate st3r_align_run_opts; the constants come from the source, the thresholds are
    checked on both sides."""
    src = open(SRC).read()
    assert re.search(r"#define MAXC 256\b", src) and re.search(r"#define CAM_STRIDE 24\b", src) and re.search(r"#define ACC_STRIDE 20\b", src)
    assert "ceil_div(ceil_div(max_rows, 256), 1024)" in src and "ceil_div(rows, 256 * rpt)" in src
    assert "n_part > 32 ? -1 : n_part" in src and "constexpr int INFL = 32;" in src
    assert "(n_corr > n_c2d ? n_corr : n_c2d) + n_dust" in src
    assert "sizeof(float) * (4 * ((size_t)C * ACC_STRIDE + 1) + (size_t)C * CAM_STRIDE)" in src and "sh > 64 * 1024" in src
    assert "C > 0 && C <= MAXC" in src
    assert (ac.ROWS_PER_WG, ac.MAX_WG, ac.MAX_INLINE_PARTIALS, ac.MAXC) == (256, 1024, 32, 256)
    L = ac.launch_shape
    assert L(0, 0, 0, 1) == (1, 0, False) and L(1, 1, 0, 1) == (1, 1, False)
    assert L(256, 0, 0, 1) == (1, 1, False) and L(257, 0, 0, 1) == (1, 2, False)
    assert L(32 * 256, 0, 0, 1) == (1, 32, False) and L(32 * 256 + 1, 0, 0, 1) == (1, 33, True)
    assert L(262144, 0, 0, 1) == (1, 1024, True) and L(262145, 0, 0, 1) == (2, 513, True)
    assert L(262144, 0, 1, 1) == (2, 513, True)                      # regression rows count
    assert L(300000, 5000, 0, 1) == (2, 586, True) and L(300000, 5000, 0, 2) == (2, 10, False)
    assert L(0, 100, 50, 1) == (1, 1, False) and L(0, 100, 50, 2) == (1, 1, False)
    # dynamic LDS: 416 C + 16 bytes; 157 views fit the default 64 KiB, 158 do not; 256 views fit the 160 KiB of a CU
    assert ac.lds_bytes(1) == 432 and all(ac.lds_bytes(c) == 416 * c + 16 for c in (2, 157, 158, 256))
    assert ac.lds_bytes(157) <= 65536 < ac.lds_bytes(158) and ac.lds_bytes(256) <= 160 * 1024
    assert "from 158 views on (157 still fit)" in src


def test_the_case_list_covers_what_it_names():
    # the one stated exception to the floor of 5e-5: stage 2 on the two 255-edge chains (see align_cases._views_case)
    odd = {n: ac.get(n).grad_floor for n in ALL if ac.get(n).grad_floor != ac.GRAD_FLOOR}
    assert odd == {"views_c255_s2": 2.6e-4, "views_c256_s2": 4.3e-4}
    # and the one case admitted with a float32 oracle off by more than 2e-3 / 4 (rows divided by the clamped 1e-3)
    assert [n for n in ALL if "max_bound" in ac.get(n).expect] == ["clamp_behind_s2"]
    rows = {ac.get(f"rows_{n}_s{s}").rows for n in (1, 63, 64, 65, 255, 256, 257) for s in (1, 2)}
    assert rows == {1, 63, 64, 65, 255, 256, 257}
    assert {ac.get(f"wg_{w}_s{s}").shape[1] for w in (31, 32, 33, 40, 41) for s in (1, 2)} == {31, 32, 33, 40, 41}
    # the 8-wide loop of k_align_reduce: a tail of 1 (33, 41) and of 0 (40); 31 / 32 stay with k_align_update
    assert 33 % 8 == 1 and 41 % 8 == 1 and 40 % 8 == 0
    assert {ac.get(f"views_c{c}_s1").C for c in (1, 2, 63, 64, 65, 157, 158, 255, 256)} == {1, 2, 63, 64, 65, 157, 158, 255, 256}
    for n in ALL:
        assert ac.get(n).C <= ac.MAXC


@pytest.mark.parametrize("name", ALL)
def test_case_is_what_it_names(name):
    c = ac.get(name)
    f, e = c.flat, c.expect
    rpt, n_part, reduce = c.shape
    for k, v in (("rows", c.rows), ("n_part", n_part), ("rpt", rpt), ("reduce", reduce), ("n_dust", c.n_dust),
                 ("n_main", c.rows - c.n_dust), ("views", c.C)):
        if k in e:
            assert e[k] == v, (k, e[k], v)
    assert n_part <= ac.MAX_WG and (c.rows == 0 or (n_part - 1) * rpt * 256 < c.rows <= n_part * rpt * 256)
    # the layout: indices inside their arrays, anchors inside their images, the drawn ranges
    A, G = len(f["anchor_idx"]), f["core_depth"].shape[1]
    assert f["anchor_idx"].min() >= 0 and f["anchor_idx"].max() < G and 64 <= G <= 257
    assert f["anchor_img"].min() >= 0 and f["anchor_img"].max() < c.C
    for k in ("corr_a1", "corr_a2", "c2d_a2", "dust_a1"):
        assert f[k].size == 0 or (f[k].min() >= 0 and f[k].max() < A), k
    for k in ("c2d_img1", "dust_img2"):
        assert f[k].size == 0 or (f[k].min() >= 0 and f[k].max() < c.C), k
    assert (f["anchor_pix"] >= 0).all() and (f["anchor_pix"] <= f["imsizes"][f["anchor_img"]] - 1).all()
    assert 0.5 <= f["anchor_offset"].min() and f["anchor_offset"].max() <= 1.1
    assert 0.5 <= f["core_depth"].min() and f["core_depth"].max() <= 2.0
    for k in ("corr_conf", "c2d_conf", "dust_conf"):
        assert f[k].size == 0 or (0.1 <= f[k].min() and f[k].max() <= 1.0)
    # the tree
    root, edges = int(f["mst_root"]), [tuple(int(x) for x in r) for r in f["mst_edges"]]
    depth = ac.tree_depth(root, edges, c.C)
    assert len(edges) == c.C - 1
    if "root" in e:
        assert root == e["root"] and depth == e["depth"], (root, depth)
    # ties of the minimum size, and how far the runner-up is
    ties, gap = ac.tie_count(c)
    assert ties == e.get("ties", 1) and (ties == c.C or gap > 1 + 1e-4), (ties, gap)
    # the focal clamp: nobody near a limit; nobody beyond one unless planted
    lo, hi = ac.focal_state(c)
    assert (np.abs(lo - 1) > 1e-3).all() and (np.abs(hi - 1) > 1e-3).all()
    assert sorted(np.nonzero((lo < 1) | (hi > 1))[0].tolist()) == e.get("fclip", [])
    if "cams_per_wave" in e:
        assert ac.cameras_per_wave(c) == e["cams_per_wave"]
        assert (f["anchor_img"][f["corr_a1"][:64]] == f["anchor_img"][f["corr_a2"][:64]]).all()   # a pair inside one image
    if "reads_view0" in e:
        reads = ac.depth_reads(c)
        assert {k: int(reads[0, k]) for k in e["reads_view0"]} == e["reads_view0"]
        assert ((f["anchor_img"] == 0) & (f["anchor_idx"] == 9)).sum() == 2
    if "elems" in e:
        assert c.C * G == e["elems"]
    # per-row values of the float64 oracle: away from every branch threshold
    R = ac.reference(name)
    d3, dd = ac.rows3d(c, R["f64"])
    assert (dd > 1e-3).all()
    if c.stage == 1:
        assert ((d3 > 1e-3) | (d3 == 0)).all() and int((d3 == 0).sum()) == e.get("zero_rows", 0)
    else:
        rz, u, v, d = ac.rows2d(c, R["f64"])
        assert ac.threshold_margin(rz, u, v) > 1e-3 and (d > 1e-3).all()
    assert np.isfinite(R["f64"]["loss"]) and (c.rows == 0) == (R["f64"]["loss"] == 0)
    if c.check:
        c.check(c, R)


@pytest.mark.parametrize("name", ALL)
def test_bounds_from_the_float32_oracle_stay_under_their_cap(name):
    """The yardstick: float32 autograd of the oracle against float64 on the case, per parameter group.  The bound of the
    GPU test is 4 x this, floored at 5e-5; a case on which that bound would pass the older tests' 2e-3 is too
    ill-conditioned to check much and is admitted only with a cap it states itself (`max_bound`: `clamp_behind_s2`)."""
    c = ac.get(name)
    R = ac.reference(name)
    worst = 0.0
    for g, (scale, yard, bound) in ac.grad_bounds(R, c.trainable(), c.grad_floor).items():
        assert bound <= c.expect.get("max_bound", 2e-3), (g, scale, yard, bound)
        worst = max(worst, yard)
    scale, yard, bound = ac.group_bound(R["f64"]["grads"]["core_depth"], R["f32"]["grads"]["core_depth"], ac.GRAD_FLOOR)
    assert bound <= c.expect.get("max_bound", 2e-3)
    for k, (scale, yard, bound) in ac.table_bounds(R).items():
        assert bound <= 1e-3, (k, yard, bound)
    assert abs(R["f32"]["loss"] - R["f64"]["loss"]) <= ac.LOSS_RTOL * abs(R["f64"]["loss"])
    print(name, "float32 oracle worst gradient error %.2e" % worst)


def test_nan_problems_have_the_workgroups_they_name():
    for wgs, stage in ((10, 2), (33, 1)):
        clean, bad, _ = ac.nan_case(wgs, stage)
        n = len(clean["corr_a1"])
        assert ac.launch_shape(n, n, 0, stage) == (1, wgs, wgs > 32)
        assert sum(int(np.isnan(bad[k]).sum()) for k in bad if bad[k].dtype.kind == "f") == 1
        assert not any(np.isnan(clean[k]).any() for k in clean if clean[k].dtype.kind == "f")


def test_schedule_values_equal_the_built_in_cosine():
    """lr1 = 2^-4 and lr2 = 2^-6 are exact in binary32, so the library's cosine (evaluated in double from the float
    argument) and the oracle's callable give the same float32 learning rates: the GPU test may then ask for equal bits."""
    from oracle import align_oracle as ao
    for lr, n in ((0.0625, 3), (0.015625, 1)):
        for it in range(n):
            built_in = np.float32(0.0 + (float(np.float32(lr)) - 0.0) * (1.0 + np.cos((it / n) * np.pi)) / 2.0)
            assert np.float32(ao.cosine_schedule(it / n, lr, 0)) == built_in
