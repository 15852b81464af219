"""CPU-only: the host side of the per-view exposures -- the argument checks of render_3dgs(exposure=...),
render_3dgs_original(exposure=True) and run_3dgs_optim(exposure_lr=..., exposure_freeze=...) that run before any GPU work,
the argument lists that reach gs.py, and the signature users program against."""
import inspect

import numpy as np
import pytest
import torch


def _scene(n=2, H=6, W=8):
    import starst3r_amd as st
    scene = st.Scene(device="cpu")
    scene.imgs = [np.zeros((H, W, 3), np.float32) for _ in range(n)]
    scene.c2w = torch.eye(4).repeat(n, 1, 1)
    scene.intrinsics = torch.eye(3).repeat(n, 1, 1)
    scene.gaussians = {"means": torch.zeros(4, 3)}
    return scene


def test_run_3dgs_optim_keeps_the_reference_order_with_the_new_keywords_last():
    from starst3r_amd import gs
    import starst3r_amd as st
    names = ["scene", "iters", "enable_pruning", "loss_ssim_fac", "loss_opacity_fac", "loss_scale_fac", "verbose", "pose_lr",
             "pose_freeze", "depth_fac", "depth_conf_thres", "exposure_lr", "exposure_freeze"]
    sig = inspect.signature(gs.run_3dgs_optim)
    assert list(sig.parameters) == names
    assert sig.parameters["exposure_lr"].default == 0.0 and sig.parameters["exposure_freeze"].default == ()
    assert list(inspect.signature(st.Scene.run_3dgs_optim).parameters) == ["self"] + names[1:]
    for fn in (gs.render_3dgs, st.Scene.render_3dgs):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["render_mode", "exposure"] and p["exposure"].default is None
    for fn in (gs.render_3dgs_original, st.Scene.render_3dgs_original):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["render_mode", "exposure"] and p["exposure"].default is False


def test_a_wrong_exposure_shape_is_refused_before_anything_runs():
    scene = _scene()
    w2c, K = scene.w2c, scene.intrinsics
    for bad in (torch.zeros(2, 3, 3), torch.zeros(3, 3, 4), torch.zeros(3, 4), torch.zeros(2, 4, 3), np.zeros((2, 3, 4)), 1.0):
        with pytest.raises(ValueError, match="exposure"):
            scene.render_3dgs(w2c, K, 8, 6, exposure=bad)
        with pytest.raises(ValueError, match="exposure"):
            scene.render_3dgs(w2c, K, 8, 6, render_mode="RGB+ED", exposure=bad)


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_depth_only_modes_take_no_exposure(mode):
    scene = _scene()
    with pytest.raises(ValueError, match="render_mode"):
        scene.render_3dgs(scene.w2c, scene.intrinsics, 8, 6, render_mode=mode, exposure=torch.zeros(2, 3, 4))
    scene.exposures = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="render_mode"):
        scene.render_3dgs_original(8, 6, render_mode=mode, exposure=True)


def test_exposure_true_needs_trained_exposures():
    scene = _scene()
    assert not hasattr(scene, "exposures")
    with pytest.raises(ValueError, match="exposures"):
        scene.render_3dgs_original(8, 6, exposure=True)
    with pytest.raises(ValueError, match="exposures"):
        scene.render_3dgs_original(8, 6, render_mode="RGB+D", exposure=True)


def test_the_delegates_pass_the_exposure_through(monkeypatch):
    from starst3r_amd import scene as scene_mod
    scene = _scene()
    calls = []
    monkeypatch.setattr(scene_mod._gs, "render_3dgs", lambda *a, **k: calls.append((a, k)) or "img")
    E = torch.zeros(2, 3, 4)
    scene.render_3dgs(scene.w2c, scene.intrinsics, 8, 6)
    assert calls[-1] == ((scene, scene.w2c, scene.intrinsics, 8, 6), {})   # the reference's call, argument for argument
    scene.render_3dgs(scene.w2c, scene.intrinsics, 8, 6, exposure=E)
    assert calls[-1][1]["exposure"] is E and calls[-1][1]["render_mode"] == "RGB"
    scene.exposures = E
    assert scene.render_3dgs_original(8, 6, render_mode="RGB+ED", exposure=True) == "img"
    assert calls[-1][1]["exposure"] is E and calls[-1][1]["render_mode"] == "RGB+ED"
    scene.render_3dgs_original(8, 6)
    assert calls[-1][1] == {}


def test_exposure_arguments_reach_the_loop_only_when_on(monkeypatch):
    from starst3r_amd import scene as scene_mod
    scene = _scene()
    calls = []
    monkeypatch.setattr(scene_mod._gs, "run_3dgs_optim", lambda *a, **k: calls.append((a, k)) or [])
    scene.run_3dgs_optim(3, exposure_lr=0.0, exposure_freeze=(0,))
    assert calls[-1] == ((scene, 3, False, 0.2, 0.01, 0.01, False), {})   # off: the reference's call
    scene.run_3dgs_optim(3, exposure_lr=1e-3, exposure_freeze=(0,))
    assert calls[-1][1] == dict(pose_lr=0.0, pose_freeze=(), depth_fac=0.0, depth_conf_thres=1.5, exposure_lr=1e-3,
                                exposure_freeze=(0,))
    rate = lambda step: 1e-3
    scene.run_3dgs_optim(3, exposure_lr=rate)
    assert calls[-1][1]["exposure_lr"] is rate


def test_exposure_freeze_indices():
    from starst3r_amd import gs
    assert gs._exposure_frozen(4, ()) == [] and gs._exposure_frozen(4, (2, 0, 2)) == [0, 2]
    assert gs._exposure_frozen(4, (-1, np.int64(1))) == [1, 3]
    for bad in ((4,), (-5,), (0.5,), (True,), (0, 7)):
        with pytest.raises(ValueError, match="exposure_freeze"):
            gs._exposure_frozen(4, bad)
    # run_3dgs_optim refuses them before anything runs (no GPU here: anything further would raise something else)
    scene = _scene()
    with pytest.raises(ValueError, match="exposure_freeze"):
        gs.run_3dgs_optim(scene, 1, exposure_lr=1e-3, exposure_freeze=(2,))
    assert not hasattr(scene, "exposures")


def test_exposure_lr_is_refused_under_the_multi_gpu_settings(monkeypatch):
    from starst3r_amd import dist as sdist, gs
    scene = _scene()
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        gs.run_3dgs_optim(scene, 1, exposure_lr=1e-3)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 1))
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError):
        gs.run_3dgs_optim(scene, 1, exposure_lr=lambda step: 1e-3)
    assert not hasattr(scene, "exposures")
