"""CPU-only: the host side of scene.backgrounds and scene.alpha_fac / alpha_masks / alpha_weights -- the checks of
run_3dgs_optim and render_3dgs that run before any GPU work (every `ops` call is replaced by one that fails the test), what
leaves the options off, the refusal under the multi-GPU settings, and the signatures users program against."""
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


@pytest.fixture
def no_ops(monkeypatch):
    """every public function of starst3r_amd.ops fails the test when called"""
    from starst3r_amd import ops

    def forbid(name):
        def f(*a, **k):
            raise AssertionError(f"ops.{name} was called before the checks were through")
        return f
    for name, fn in list(vars(ops).items()):
        if inspect.isfunction(fn) and not name.startswith("_"):
            monkeypatch.setattr(ops, name, forbid(name))


def test_the_signatures(no_ops):
    from starst3r_amd import gs
    import starst3r_amd as st
    names = ["scene", "iters", "enable_pruning", "loss_ssim_fac", "loss_opacity_fac", "loss_scale_fac", "verbose", "pose_lr",
             "pose_freeze", "depth_fac", "depth_conf_thres", "exposure_lr", "exposure_freeze"]
    assert list(inspect.signature(gs.run_3dgs_optim).parameters) == names          # settings of the scene, no arguments
    assert list(inspect.signature(st.Scene.run_3dgs_optim).parameters) == ["self"] + names[1:]
    for word in ("scene.backgrounds", "scene.alpha_fac", "alpha_masks", "alpha_weights"):
        assert word in gs.run_3dgs_optim.__doc__, word
    # the render's backgrounds are a setting of the scene as well: the argument lists are the parent's, slot for slot
    for fn, head in ((gs.render_3dgs, ["scene"]), (st.Scene.render_3dgs, ["self"])):
        p = inspect.signature(fn).parameters
        assert list(p) == head + ["w2c", "intrinsics", "width", "height", "render_mode", "exposure"]
        assert p["render_mode"].default == "RGB" and p["exposure"].default is None
    for fn, head in ((gs.render_3dgs_original, ["scene"]), (st.Scene.render_3dgs_original, ["self"])):
        p = inspect.signature(fn).parameters
        assert list(p) == head + ["width", "height", "render_mode", "exposure"]
        assert p["render_mode"].default == "RGB" and p["exposure"].default is False
    assert "scene.render_backgrounds" in gs.render_3dgs.__doc__


BAD_BACKGROUNDS = {
    "count": lambda: np.ones((3, 3), np.float32),
    "shape": lambda: np.ones((2, 4), np.float32),
    "flat": lambda: torch.ones(6),
    "scalar": lambda: 1.0,
    "nan": lambda: np.array([[1.0, np.nan, 1.0], [0, 0, 0]]),
    "inf": lambda: torch.tensor([[1.0, 1.0, 1.0], [0, float("inf"), 0]]),
    "bool": lambda: np.ones((2, 3), bool),
    "text": lambda: "white",
}


@pytest.mark.parametrize("kind", sorted(BAD_BACKGROUNDS))
def test_bad_backgrounds_raise_value_error_before_anything_runs(no_ops, kind):
    from starst3r_amd import gs
    scene = _scene()
    scene.backgrounds = BAD_BACKGROUNDS[kind]()
    with pytest.raises(ValueError, match="backgrounds"):
        gs.run_3dgs_optim(scene, 1)
    assert getattr(scene, "_backgrounds_dev", None) is None


H, W = 6, 8
BAD_ALPHA = {
    # name: (alpha_fac, alpha_masks, alpha_weights, the word the message must hold)
    "fac_without_masks": lambda: (1.0, None, None, "alpha_masks"),
    "fac_nan": lambda: (float("nan"), [np.ones((H, W)), None], None, "alpha_fac"),
    "fac_inf": lambda: (float("inf"), None, None, "alpha_fac"),
    "fac_callable": lambda: (lambda step: 1.0, [np.ones((H, W)), None], None, "alpha_fac"),
    "fac_text": lambda: ("1", [np.ones((H, W)), None], None, "alpha_fac"),
    "count": lambda: (1.0, [np.ones((H, W))], None, "alpha_masks"),
    "not_a_list": lambda: (1.0, np.ones((2, H, W)), None, "alpha_masks"),
    "shape": lambda: (1.0, [None, np.ones((W, H))], None, "alpha_masks"),
    "no_shape": lambda: (1.0, [None, 1.0], None, "alpha_masks"),
    "above_one": lambda: (1.0, [np.full((H, W), 1.5), None], None, "alpha_masks"),
    "negative": lambda: (1.0, [None, -torch.ones(H, W)], None, "alpha_masks"),
    "nan": lambda: (1.0, [np.where(np.eye(H, W) > 0, np.nan, 1.0), None], None, "alpha_masks"),
    "checked_with_fac_zero": lambda: (0.0, [np.full((H, W), 2.0), None], None, "alpha_masks"),
    "w_count": lambda: (1.0, [np.ones((H, W)), None], [None], "alpha_weights"),
    "w_shape": lambda: (1.0, [np.ones((H, W)), None], [np.ones((H, W, 1)), None], "alpha_weights"),
    "w_negative": lambda: (1.0, [np.ones((H, W)), None], [np.full((H, W), -1.0), None], "alpha_weights"),
    "w_inf": lambda: (1.0, [np.ones((H, W)), None], [None, torch.full((H, W), float("inf"))], "alpha_weights"),
    "w_not_a_list": lambda: (1.0, [np.ones((H, W)), None], np.ones((2, H, W)), "alpha_weights"),
}


@pytest.mark.parametrize("kind", sorted(BAD_ALPHA))
def test_bad_alpha_settings_raise_value_error_before_anything_runs(no_ops, kind):
    from starst3r_amd import gs
    scene = _scene()
    scene.alpha_fac, scene.alpha_masks, scene.alpha_weights, word = BAD_ALPHA[kind]()
    with pytest.raises(ValueError, match=word):
        gs.run_3dgs_optim(scene, 1)
    # before the other options' side effects too
    with pytest.raises(ValueError, match=word):
        gs.run_3dgs_optim(scene, 1, exposure_lr=1e-3)
    assert not hasattr(scene, "exposures") and getattr(scene, "_alpha_maps_dev", None) is None


def test_the_off_settings_build_no_option(no_ops):
    from starst3r_amd import gs
    scene = _scene()
    on = lambda: gs._AlphaMasks.when_on(scene, False, getattr(scene, "alpha_fac", 0.0), getattr(scene, "alpha_masks", None),
                                        getattr(scene, "alpha_weights", None))
    assert gs._Backgrounds.when_on(scene, False, getattr(scene, "backgrounds", None)) is None and on() is None
    scene.backgrounds = None
    assert gs._Backgrounds.when_on(scene, False, scene.backgrounds) is None
    scene.alpha_masks = [np.ones((H, W), bool), None]                # masks without a factor: off
    assert on() is None
    scene.alpha_fac = 0.0
    assert on() is None
    scene.alpha_fac, scene.alpha_masks = 0.5, [None, None]           # nothing to supervise: off
    assert on() is None
    scene.alpha_masks = [np.ones((H, W), bool), None]
    o = on()
    assert isinstance(o, gs._AlphaMasks) and isinstance(o, gs._PerViewOption) and o.fac == 0.5 and o.masks is scene.alpha_masks
    for b in (np.ones((2, 3)), torch.zeros(2, 3), [[1, 1, 1], [0, 0, 0]], np.ones((2, 3), np.uint8)):
        o = gs._Backgrounds.when_on(scene, False, b)
        assert isinstance(o, gs._Backgrounds) and isinstance(o, gs._PerViewOption)


def test_the_uploads_are_float32_stacked_and_cached(no_ops):
    import types
    from starst3r_amd import gs
    scene = _scene(n=3)
    m0, w2 = np.zeros((H, W), bool), torch.full((H, W), 0.5, dtype=torch.float64)
    scene.alpha_fac, scene.alpha_masks, scene.alpha_weights = 1.0, [m0, None, torch.ones(H, W)], [None, np.ones((H, W)), w2]
    c = types.SimpleNamespace(scene=scene, views=[0, 1, 2], height=H, width=W)
    o = gs._AlphaMasks.when_on(scene, False, scene.alpha_fac, scene.alpha_masks, scene.alpha_weights)
    o.set_up(c)
    for t in (o.target, o.weights):
        assert t.dtype == torch.float32 and tuple(t.shape) == (3, H, W) and t.is_contiguous()
    assert torch.all(o.target[0] == 0) and torch.all(o.target[1] == 0) and torch.all(o.target[2] == 1)
    # no weights entry: ones; no target: weight 0 whatever alpha_weights holds; a weight map: itself
    assert torch.all(o.weights[0] == 1) and torch.all(o.weights[1] == 0) and torch.all(o.weights[2] == 0.5)
    first = o.target
    o2 = gs._AlphaMasks.when_on(scene, False, scene.alpha_fac, scene.alpha_masks, scene.alpha_weights)
    o2.set_up(c)
    assert o2.target is first                                        # cached
    w2[0, 0] = 2.0                                                   # a tensor edited in place
    o3 = gs._AlphaMasks.when_on(scene, False, scene.alpha_fac, scene.alpha_masks, scene.alpha_weights)
    o3.set_up(c)
    assert o3.target is not first and o3.weights[2, 0, 0] == 2.0
    c.views = [0, 2]
    o3.set_up(c)
    assert o3.target.shape[0] == 2
    scene.backgrounds = np.array([[1, 1, 1], [0, 0.5, 0], [0.25, 0, 0]], np.float64)
    b = gs._Backgrounds.when_on(scene, False, scene.backgrounds)
    b.set_up(c)
    assert b.colors.dtype == torch.float32 and b.colors.tolist() == [[1, 1, 1], [0.25, 0, 0]] and b.colors.is_contiguous()
    kept = b.colors
    b2 = gs._Backgrounds.when_on(scene, False, scene.backgrounds)
    b2.set_up(c)
    assert b2.colors is kept


@pytest.mark.parametrize("which", ["backgrounds", "alpha"])
def test_both_options_are_refused_under_the_multi_gpu_settings(no_ops, monkeypatch, which):
    from starst3r_amd import dist as sdist, gs
    scene = _scene()
    if which == "backgrounds":
        scene.backgrounds = np.ones((2, 3), np.float32)
    else:
        scene.alpha_fac, scene.alpha_masks = 1.0, [np.ones((H, W), np.float32), None]
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=which):
        gs.run_3dgs_optim(scene, 1)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 1))
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError, match=which):
        gs.run_3dgs_optim(scene, 1)


def test_render_checks_come_before_anything_runs(no_ops):
    scene = _scene()
    w2c, K = scene.w2c, scene.intrinsics
    for bad in (torch.zeros(2, 4), torch.zeros(3, 3), torch.zeros(3), np.zeros((2, 3)), 1.0, "white"):
        scene.render_backgrounds = bad
        with pytest.raises(ValueError, match="render_backgrounds"):
            scene.render_3dgs(w2c, K, 8, 6)
        with pytest.raises(ValueError, match="render_backgrounds"):
            scene.render_3dgs(w2c, K, 8, 6, "RGB+ED")               # render_mode keeps its positional slot
    scene.render_backgrounds = torch.zeros(2, 3)
    for mode in ("D", "ED"):
        with pytest.raises(ValueError, match="render_mode"):
            scene.render_3dgs(w2c, K, 8, 6, render_mode=mode)
    scene.render_backgrounds = True
    with pytest.raises(ValueError, match="scene.backgrounds"):
        scene.render_3dgs_original(8, 6)                            # there are none
    scene.backgrounds = np.ones((2, 3), np.float32)
    with pytest.raises(ValueError, match="render_mode"):
        scene.render_3dgs_original(8, 6, "D")
    with pytest.raises(ValueError, match="render_backgrounds"):
        scene.render_3dgs(w2c[:1], K[:1], 8, 6)                     # True stands for one colour per image of the scene


def test_the_setting_reaches_the_composite_and_off_reaches_nothing(monkeypatch):
    """_render_backgrounds: None / False / absent are off; a tensor is passed on as it is (so that it can take a gradient);
    True stands for scene.backgrounds as float32"""
    from starst3r_amd import gs
    scene = _scene()
    assert gs._render_backgrounds(scene, 2, "RGB") is None          # absent
    for off in (None, False):
        scene.render_backgrounds = off
        assert gs._render_backgrounds(scene, 2, "RGB") is None and gs._render_backgrounds(scene, 2, "D") is None
    B = torch.ones(2, 3, requires_grad=True)
    scene.render_backgrounds = B
    assert gs._render_backgrounds(scene, 2, "RGB") is B and gs._render_backgrounds(scene, 2, "RGB+ED") is B
    scene.render_backgrounds = True
    scene.backgrounds = [[1, 1, 1], [0, 0, 0]]
    got = gs._render_backgrounds(scene, 2, "RGB+D")
    assert got.dtype == torch.float32 and torch.equal(got, torch.tensor([[1.0, 1, 1], [0, 0, 0]]))
