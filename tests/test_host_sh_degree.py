"""CPU: the SH cases reach the edges they name, their float32 restatement is the autograd reference's chain rule, and the
settings are validated before anything runs (no GPU).

The first three tests (test_cases_reach_their_edges, test_restatement_is_the_reference_chain_rule, test_degrees_nest) check
the fixtures of tests/sh_cases.py themselves and touch no code of the package: they pass whatever the library does.  The
tests below "settings" are the ones that fail without the feature."""
import types

import numpy as np
import pytest
import torch

import sh_cases as sc


@pytest.mark.parametrize("Cn", sc.CS)
def test_cases_reach_their_edges(Cn):
    case = sc.get(257, Cn)
    cp = sc.campos_of(case.viewmats)
    u, inrm = sc.directions(case.means, cp)
    vis, tags = case.vis, case.tags
    assert vis.sum(1).min() >= 8 and not vis.all() or Cn == 1
    if Cn <= 2:      # straight ahead of the planted camera; one coordinate zero
        (g,) = tags["axis"]
        assert vis[0, g] and tuple(u[0, g]) == (0.0, 0.0, 1.0)
        b = sc.basis(*u[0, g], 3)
        assert [i for i in range(16) if b[i] == 0.0] == [1, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15]
        assert any(vis[0, g] and u[0, g, 0] == 0.0 and u[0, g, 1] != 0.0 for g in tags["plane"])
        assert any(vis[0, g] and u[0, g, 1] == 0.0 and u[0, g, 0] != 0.0 for g in tags["plane"])
    else:            # along -x from ring camera 0, along +y from the camera that looks down the y axis: exact zeros
        gx, gy = tags["axis"]
        u32, _ = sc.directions(case.means, cp, np.float32)
        for uu in (u, u32):
            assert vis[0, gx] and uu[0, gx, 0] < -0.999999 and uu[0, gx, 1] == 0.0 and uu[0, gx, 2] == 0.0
            assert vis[sc.Y_CAM, gy] and uu[sc.Y_CAM, gy, 1] > 0.999999 and uu[sc.Y_CAM, gy, 0] == 0.0 and uu[sc.Y_CAM, gy, 2] == 0.0
        b = sc.basis(*u[sc.Y_CAM, gy], 3)     # on the y axis only rows 0, 1, 6, 8, 9, 11 are not zero
        assert [i for i in range(16) if b[i] == 0.0] == [2, 3, 4, 5, 7, 10, 12, 13, 14, 15]
    (g,) = tags["close"]
    assert vis[Cn - 1, g] and 900.0 < inrm[Cn - 1, g] < 1100.0
    for g in tags["culled"]:
        assert vis[:, g].any() and not vis[:, g].all()
    assert Cn == 1 or len(tags["culled"]) == 2
    for deg in sc.DEGREES:
        assert sc.clamped_counts(case, deg) == {0, 1, 2, 3}
        p = sc.pre_clamp(case.means, cp, case.sh, deg)
        assert np.abs(p[vis]).min() >= sc.MARGIN
        if deg >= 1 and Cn > 1:   # a channel clamped in one view and not in another
            assert ((p < 0).any(0) & (p >= 0).any(0) & vis.all(0)[:, None]).any()


@pytest.mark.parametrize("deg", sc.DEGREES)
def test_restatement_is_the_reference_chain_rule(deg):
    """in float64 the written-out chain rule (basis_grad, tangent projection, the finish through inverse(V)) agrees with
    autograd to rounding: the float32 bounds measure arithmetic, not a formula"""
    case = sc.get(255, 2)
    v = sc.colour_cotangents(case)
    r, o = sc.ref64(case, deg, v), sc.restate(case, deg, v, np.float64)
    for g in sc.GROUPS:
        assert np.abs(o[g] - r[g]).max() <= 1e-9 * max(np.abs(r[g]).max(), 1.0), g
    assert np.abs(o["colour"][case.vis] - r["colour"][case.vis]).max() <= 1e-12
    if deg >= 1:
        assert np.abs(r["means"]).max() > 0 and np.abs(r["viewmats"]).max() > 0
    b = sc.reference(255, 2, deg)["bounds"]
    for g in sc.GROUPS:
        assert sc.FLOOR <= b[g]["rel"] < 1e-2, (g, b[g]["rel"])


def test_degrees_nest():
    """rows above a degree zero: the higher degree's colour is the lower one's"""
    case = sc.get(255, 2)
    cp = sc.campos_of(case.viewmats)
    for lo in (0, 1, 2):
        sh = case.sh.copy(); sh[:, sc.rows(lo):] = 0
        assert np.array_equal(sc.pre_clamp(case.means, cp, sh, 3), sc.pre_clamp(case.means, cp, sh, lo))


# ---------------------------------------------------------------------------------------------------------------------
# settings
def test_scene_sh_degree_values():
    from starst3r_amd import gs
    assert gs._sh_degree(types.SimpleNamespace()) is None
    assert gs._sh_degree(types.SimpleNamespace(sh_degree=None)) is None
    for d in (0, 1, 2, 3):
        assert gs._sh_degree(types.SimpleNamespace(sh_degree=d)) == d
    assert gs._sh_degree(types.SimpleNamespace(sh_degree=np.int64(2))) == 2
    for bad in (True, False, 4, -1, 2.0, "3", (1,)):
        with pytest.raises(ValueError, match="sh_degree"):
            gs._sh_degree(types.SimpleNamespace(sh_degree=bad))


def test_render_checks_the_setting_before_anything_runs():
    from starst3r_amd import gs
    scene = types.SimpleNamespace(sh_degree=True)     # no gaussians, no device: the check comes first
    with pytest.raises(ValueError, match="sh_degree"):
        gs.render_3dgs(scene, torch.eye(4)[None], torch.eye(3)[None], 8, 8)


def test_ops_set_sh_degree_refusals():
    """ValueError before the library is touched (a stand-in ctx without a handle would raise AttributeError otherwise)"""
    from starst3r_amd import ops
    ctx = types.SimpleNamespace()
    assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT == (1, 1, None)
    for deg, act in ((4, None), (-1, None), (True, None), (2.0, None), (2, 3), (2, -1), (3, True), (1, 2)):
        with pytest.raises(ValueError, match="degree"):
            ops.set_sh_degree(ctx, deg, act)
    with pytest.raises(ValueError, match="v_sh_high"):
        ops.set_sh_degree(ctx, 1, 1, torch.zeros(4, 15))
    with pytest.raises(ValueError, match="v_sh_high"):
        ops.set_sh_degree(ctx, 3, 3, torch.zeros(4, 15))          # degree 3 holds 36 floats per Gaussian
    assert [ops.sh_rows(d) for d in range(4)] == [1, 4, 9, 16]
    assert ops.get_sh_degree(ctx) == ops.SH_DEFAULT


def test_interval_schedule_arithmetic():
    """gsplat's trainer: sh_degree_to_use = min(step // interval, sh_degree) with its 0-based step = our counter t - 1"""
    from starst3r_amd import gs
    assert [gs._sh_active_degree(t, 0, 3) for t in (1, 2, 1000)] == [3, 3, 3]
    assert [gs._sh_active_degree(t, 1000, 3) for t in (1, 1000, 1001, 2000, 2001, 3000, 3001, 10 ** 6)] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert [gs._sh_active_degree(t, 2, 2) for t in range(1, 9)] == [0, 0, 1, 1, 2, 2, 2, 2]
    assert [gs._sh_active_degree(t, 1, 0) for t in (1, 5)] == [0, 0]


def test_run_3dgs_optim_checks_the_settings_before_anything_runs():
    from starst3r_amd import gs
    for bad in (dict(sh_degree=True), dict(sh_degree=4), dict(sh_degree="2"),
                dict(sh_degree=2, sh_degree_interval=-1), dict(sh_degree=2, sh_degree_interval=1.5),
                dict(sh_degree=2, sh_degree_interval=True), dict(sh_degree=2, sh_high_lr=-1e-3),
                dict(sh_degree=2, sh_high_lr="fast")):
        scene = types.SimpleNamespace(**bad)            # no images, no Gaussians: the checks come first
        with pytest.raises(ValueError, match="sh_"):
            gs.run_3dgs_optim(scene, 1)
    assert gs._ShDegree.when_on(types.SimpleNamespace(sh_degree=None, sh_degree_interval="junk"), False) is None


def test_sh_degree_refusals(monkeypatch):
    from starst3r_amd import gs
    scene = types.SimpleNamespace(sh_degree=3, strategy=object())
    with pytest.raises(NotImplementedError, match="MCMCStrategy"):       # a foreign strategy does not carry the high moments
        gs._ShDegree.when_on(scene, True)
    assert gs._ShDegree.when_on(types.SimpleNamespace(sh_degree=3, strategy=gs.MCMCStrategy()), True).rows == 16
    assert gs._ShDegree.when_on(types.SimpleNamespace(sh_degree=1, strategy=object()), True).rows == 4
    assert [gs._ShDegree.when_on(types.SimpleNamespace(sh_degree=d), False).rows for d in range(4)] == [4, 4, 9, 16]
    monkeypatch.setattr(gs._dist, "rank_world", lambda: (0, 2))          # under torch.distributed: like every option
    with pytest.raises(NotImplementedError, match="scene.sh_degree"):
        gs._ShDegree.when_on(scene, False)
