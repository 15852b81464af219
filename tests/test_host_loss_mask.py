"""CPU-only: the host side of scene.loss_masks -- the checks of run_3dgs_optim that run before any GPU work, what leaves
the option off, the refusal under the multi-GPU settings, and the signature users program against."""
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


def test_the_signature_of_run_3dgs_optim_is_unchanged():
    from starst3r_amd import gs
    import starst3r_amd as st
    names = ["scene", "iters", "enable_pruning", "loss_ssim_fac", "loss_opacity_fac", "loss_scale_fac", "verbose", "pose_lr",
             "pose_freeze", "depth_fac", "depth_conf_thres", "exposure_lr", "exposure_freeze"]
    assert list(inspect.signature(gs.run_3dgs_optim).parameters) == names
    assert list(inspect.signature(st.Scene.run_3dgs_optim).parameters) == ["self"] + names[1:]
    assert "scene.loss_masks" in gs.run_3dgs_optim.__doc__


BAD = {
    "count": lambda: [np.ones((6, 8), np.float32)],
    "count_long": lambda: [None, None, np.ones((6, 8))],
    "shape": lambda: [None, np.ones((8, 6), np.float32)],
    "shape_channels": lambda: [np.ones((6, 8, 3), np.float32), None],
    "no_shape": lambda: [None, 1.0],
    "negative": lambda: [np.full((6, 8), -0.5, np.float32), None],
    "negative_tensor": lambda: [None, -torch.ones(6, 8)],
    "nan": lambda: [np.where(np.eye(6, 8) > 0, np.nan, 1.0), None],
    "inf": lambda: [None, torch.full((6, 8), float("inf"))],
    "not_a_list": lambda: np.ones((2, 6, 8), np.float32),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_masks_raise_value_error_before_anything_runs(kind):
    from starst3r_amd import gs
    scene = _scene()
    scene.loss_masks = BAD[kind]()
    with pytest.raises(ValueError, match="loss_masks"):
        gs.run_3dgs_optim(scene, 1)
    # before the other options' checks and their side effects too
    with pytest.raises(ValueError, match="loss_masks"):
        gs.run_3dgs_optim(scene, 1, exposure_lr=1e-3, exposure_freeze=(7,))
    assert not hasattr(scene, "exposures") and getattr(scene, "_loss_mask_dev", None) is None


def test_none_absent_and_all_none_leave_the_option_off():
    from starst3r_amd import gs
    scene = _scene()
    assert not hasattr(scene, "loss_masks")
    assert gs._LossMasks.when_on(scene, False, getattr(scene, "loss_masks", None)) is None
    scene.loss_masks = None
    assert gs._LossMasks.when_on(scene, False, scene.loss_masks) is None
    scene.loss_masks = [None, None]
    assert gs._LossMasks.when_on(scene, False, scene.loss_masks) is None
    for masks in ([None, np.ones((6, 8), bool)], [torch.zeros(6, 8), None], [np.ones((6, 8), np.uint8), np.ones((6, 8))]):
        scene.loss_masks = masks
        o = gs._LossMasks.when_on(scene, False, scene.loss_masks)
        assert isinstance(o, gs._LossMasks) and isinstance(o, gs._PerViewOption) and o.masks is masks


def test_the_upload_is_stacked_float32_and_cached_by_identity_and_version():
    from starst3r_amd import gs
    scene = _scene(n=3)
    a, b = np.arange(48, dtype=np.float64).reshape(6, 8), torch.ones(6, 8, dtype=torch.bool)
    scene.loss_masks = [a, None, b]
    w = gs._loss_masks_on_device(scene, scene.loss_masks, [0, 1, 2], 6, 8)
    assert w.dtype == torch.float32 and tuple(w.shape) == (3, 6, 8) and w.is_contiguous()
    assert torch.equal(w[0], torch.tensor(a, dtype=torch.float32)) and torch.all(w[1] == 1) and torch.all(w[2] == 1)
    assert gs._loss_masks_on_device(scene, scene.loss_masks, [0, 1, 2], 6, 8) is w          # cached
    b[0, 0] = False                                                                            # a tensor edited in place
    w2 = gs._loss_masks_on_device(scene, scene.loss_masks, [0, 1, 2], 6, 8)
    assert w2 is not w and w2[2, 0, 0] == 0
    scene.loss_masks = [a.copy(), None, b]                                                     # a new array
    assert gs._loss_masks_on_device(scene, scene.loss_masks, [0, 1, 2], 6, 8) is not w2
    assert gs._loss_masks_on_device(scene, scene.loss_masks, [0, 2], 6, 8).shape[0] == 2      # other views


def test_loss_masks_are_refused_under_the_multi_gpu_settings(monkeypatch):
    from starst3r_amd import dist as sdist, gs
    scene = _scene()
    scene.loss_masks = [np.ones((6, 8), np.float32), None]
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="loss_masks"):
        gs.run_3dgs_optim(scene, 1)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 1))
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError, match="loss_masks"):
        gs.run_3dgs_optim(scene, 1)
    scene.loss_masks = [None, None]   # off: the refusal does not apply (what follows needs a GPU and raises something else)
    assert gs._LossMasks.when_on(scene, False, scene.loss_masks) is None
