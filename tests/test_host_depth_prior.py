"""CPU-only: the host side of run_3dgs_optim(depth_fac=...) -- the scene's depth-map attributes, the argument list that
reaches gs.run_3dgs_optim and the checks that run before any GPU work."""
import types

import numpy as np
import pytest
import torch


def _scene(n=2, H=6, W=8):
    import starst3r_amd as st
    scene = st.Scene(device="cpu")
    scene.imgs = [np.zeros((H, W, 3), np.float32) for _ in range(n)]
    return scene


def test_scene_starts_without_depth_maps():
    scene = _scene()
    assert scene.depth_maps == [] and scene.depth_confs == []


def test_defaults_reach_the_loop_with_the_reference_arguments(monkeypatch):
    from starst3r_amd import scene as scene_mod
    scene = _scene()
    calls = []
    monkeypatch.setattr(scene_mod._gs, "run_3dgs_optim", lambda *a, **k: calls.append((a, k)) or [])
    scene.run_3dgs_optim(3)
    scene.run_3dgs_optim(3, depth_fac=0.0, depth_conf_thres=9.0)
    assert all(a == (scene, 3, False, 0.2, 0.01, 0.01, False) and k == {} for a, k in calls) and len(calls) == 2
    scene.run_3dgs_optim(3, pose_lr=1e-3)
    assert calls[-1][1] == dict(pose_lr=1e-3, pose_freeze=())
    scene.run_3dgs_optim(3, depth_fac=0.25, pose_lr=1e-3)
    assert calls[-1][1] == dict(pose_lr=1e-3, pose_freeze=(), depth_fac=0.25, depth_conf_thres=1.5)


def test_prior_upload_checks_and_weights():
    from starst3r_amd import gs
    scene = _scene()
    with pytest.raises(ValueError):
        gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)          # no maps
    scene.depth_maps = [torch.full((6, 8), 2.0), torch.full((6, 9), 2.0)]
    with pytest.raises(ValueError):
        gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)          # a map that is not its image's shape
    scene.depth_maps[1] = torch.full((6, 8), 3.0)
    z, w = gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)
    assert z.shape == (2, 6, 8) and float(z[1, 0, 0]) == 3.0 and bool((w == 1).all())   # no confidences: all ones
    assert gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)[0] is z                  # cached like the ground truth
    scene.depth_maps[1].fill_(4.0)                                                       # edited in place: uploaded again
    assert float(gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)[0][1, 0, 0]) == 4.0
    conf = torch.zeros(6, 8); conf[2] = 1.5; conf[3] = 1.6
    scene.depth_confs = [conf, conf.clone()]
    z2, w2 = gs._depth_prior_on_device(scene, [1], 1.5, 6, 8)
    assert z2.shape == (1, 6, 8) and float(w2.sum()) == 8.0 and bool((w2[0, 3] == 1).all())   # strictly above the threshold
    scene.depth_confs = [conf]
    with pytest.raises(ValueError):
        gs._depth_prior_on_device(scene, [0, 1], 1.5, 6, 8)          # confidences for some views only


def test_depth_fac_is_refused_under_the_multi_gpu_settings(monkeypatch):
    from starst3r_amd import dist as sdist, gs
    scene = _scene()
    scene.gaussians = {"means": torch.zeros(4, 3)}
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        gs.run_3dgs_optim(scene, 1, depth_fac=1.0)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 1))
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError):
        gs.run_3dgs_optim(scene, 1, depth_fac=1.0)


def test_add_images_without_dense_depth_keeps_the_lists_empty(monkeypatch):
    """a result object without get_dense_depth (Mast3r's own SparseGA): everything add_images set before is set as before"""
    from starst3r_amd import scene as scene_mod
    pts = [torch.arange(12.0).reshape(4, 3)]
    res = types.SimpleNamespace(imgs=[np.zeros((2, 2, 3), np.float32)], cam2w=torch.eye(4)[None], intrinsics=torch.eye(3)[None],
                                get_dense_pts3d=lambda clean_depth=True: (pts, None, [torch.tensor([2.0, 0.0, 2.0, 2.0])]))
    monkeypatch.setattr(scene_mod, "reconstruct_scene", lambda *a, **k: (res, {"p": 1}))
    scene = scene_mod.Scene(device="cpu")
    scene.add_images(None, [torch.zeros(3, 2, 2)])
    assert scene.depth_maps == [] and scene.depth_confs == [] and scene.dense_pts[0].shape == (3, 3)
    res.get_dense_depth = lambda: [torch.full((2, 2), 5.0)]
    scene2 = scene_mod.Scene(device="cpu")
    scene2.add_images(None, [torch.zeros(3, 2, 2)])
    assert torch.equal(scene2.depth_maps[0], torch.full((2, 2), 5.0))
    assert torch.equal(scene2.depth_confs[0], torch.tensor([[2.0, 0.0], [2.0, 2.0]]))
