"""The scene settings intrinsics_lr / intrinsics_freeze / intrinsics_tie_focal / intrinsics_opt_pp / intrinsics_grad: what
is decided before anything runs on the GPU -- the layouts that refuse the refinement, the checks of intrinsics_freeze, and
that the settings at their defaults leave the calls and scene.intrinsics alone.  No GPU needed."""
import numpy as np
import pytest
import torch

from st3r_synth import synth


def _cpu_scene(V=3, N=50, W=32, H=24):
    import starst3r_amd as st
    from starst3r_amd import gs
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=3)
    scene = st.Scene(device="cpu")
    scene.imgs = [np.zeros((H, W, 3), np.float32) for _ in range(V)]
    scene.c2w = torch.inverse(torch.tensor(w2c).double()).float()
    scene.intrinsics = torch.tensor(Ks)
    scene.gaussians = {k: torch.nn.Parameter(torch.tensor(v)) for k, v in g.items()}
    scene._gs_optim = gs._OptimState(scene, 1e-3)
    return scene


def _untouched(scene, K, before):
    st_ = scene._gs_optim
    return (scene.intrinsics is K and torch.equal(K, before) and st_.step == 0 and not hasattr(st_, "k_m")
            and not hasattr(st_, "k_step"))


def test_a_new_scene_has_the_refinement_switched_off():
    import starst3r_amd as st
    scene = st.Scene(device="cpu")
    assert scene.intrinsics_lr == 0.0 and scene.intrinsics_freeze == () and scene.intrinsics_tie_focal is True
    assert scene.intrinsics_opt_pp is False and scene.intrinsics_grad is False


def test_intrinsics_lr_under_the_gaussian_sharded_setting_is_refused(monkeypatch):
    scene = _cpu_scene()
    K, before = scene.intrinsics, scene.intrinsics.clone()
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    for rate in (1e-3, lambda step: 1e-3):
        scene.intrinsics_lr = rate
        with pytest.raises(NotImplementedError, match="intrinsics_lr"):
            scene.run_3dgs_optim(1)
    assert _untouched(scene, K, before)


def test_intrinsics_lr_under_torch_distributed_is_refused(monkeypatch):
    """world > 1: refused before any GPU work (the process group is not needed to see it: rank_world is what the loop asks)"""
    from starst3r_amd import dist as sdist
    scene = _cpu_scene()
    K, before = scene.intrinsics, scene.intrinsics.clone()
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    scene.intrinsics_lr = 1e-3
    with pytest.raises(NotImplementedError, match="intrinsics_lr"):
        scene.run_3dgs_optim(1)
    assert _untouched(scene, K, before)


@pytest.mark.parametrize("bad", [(3,), (-4,), (0, 7), (1.5,), (True,)])
def test_out_of_range_intrinsics_freeze_is_refused(bad):
    scene = _cpu_scene()
    K, before = scene.intrinsics, scene.intrinsics.clone()
    scene.intrinsics_lr, scene.intrinsics_freeze = 1e-3, bad
    with pytest.raises(ValueError, match="intrinsics_freeze"):
        scene.run_3dgs_optim(1)
    assert _untouched(scene, K, before)


def test_view_indices_count_from_the_end():
    from starst3r_amd import gs
    assert gs._view_indices(3, (-1, 0, 2, 0), "intrinsics_freeze") == [0, 2]
    assert gs._view_indices(3, (), "intrinsics_freeze") == []


def test_the_settings_do_not_change_the_calls_that_reach_gs(monkeypatch):
    """Scene hands gs.py the reference's calls, argument for argument, whatever the settings hold: gs.py reads them from
    the scene."""
    from starst3r_amd import scene as scene_mod
    scene = _cpu_scene()
    K = scene.intrinsics
    calls = []
    monkeypatch.setattr(scene_mod._gs, "run_3dgs_optim", lambda *a, **k: calls.append((a, k)) or [])
    monkeypatch.setattr(scene_mod._gs, "render_3dgs", lambda *a, **k: calls.append((a, k)) or None)
    w = torch.eye(4)[None]
    for on in (False, True):
        if on:
            scene.intrinsics_lr, scene.intrinsics_freeze, scene.intrinsics_grad = 1e-3, (0,), True
        scene.run_3dgs_optim(3)
        assert calls[-1] == ((scene, 3, False, 0.2, 0.01, 0.01, False), {})
        scene.render_3dgs(w, K[:1], 32, 24)
        assert len(calls[-1][0]) == 5 and calls[-1][1] == {}
    assert scene.intrinsics is K


def test_the_library_interface_names_the_three_exports():
    from starst3r_amd import _lib
    for name, n_args in (("st3r_gs_intrinsics_bwd", 15), ("st3r_intrinsics_adam_step", 16),
                         ("st3r_ctx_set_intrinsics_grad", 6)):
        assert len(_lib.SIGNATURES[name]) == n_args
