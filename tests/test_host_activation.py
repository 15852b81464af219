"""CPU-only: the host side of scene.activations -- the declarations and exports of the four C functions, the settings of
the scene, init_3dgs and activate_3dgs (plain torch: they run on a CPU scene), the checks that come before anything is
allocated or launched, and the refusal under the multi-GPU settings."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import activation_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("st3r_param_activate", "st3r_param_activate_bwd", "st3r_ctx_set_activation", "st3r_ctx_get_activation")


def _scene(n=2, H=6, W=8):
    import starst3r_amd as st
    scene = st.Scene(device="cpu")
    scene.imgs = [np.zeros((H, W, 3), np.float32) for _ in range(n)]
    scene.c2w = torch.eye(4).repeat(n, 1, 1)
    scene.intrinsics = torch.eye(3).repeat(n, 1, 1)
    scene.gaussians = {"means": torch.zeros(4, 3)}
    return scene


def _points(scene, n=37, seed=0):
    gen = torch.Generator().manual_seed(seed)
    scene.dense_pts = [torch.randn(n, 3, generator=gen)]
    scene.dense_cols = [torch.rand(n, 3, generator=gen)]
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


def test_the_header_declares_and_the_library_exports_the_four_functions():
    from starst3r_amd import _lib, build, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3r.h")).read(), flags=re.S)
    L = ctypes.CDLL(build.build())
    for fn in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % fn, src), fn
        assert hasattr(L, fn) and fn in _lib.SIGNATURES, fn
    for name in ("param_activate", "param_activate_bwd", "set_activation", "get_activation"):
        assert callable(getattr(ops, name))
    # the internal interface and the arena slots
    stages = open(os.path.join(ROOT, "starst3r_amd", "csrc", "stages.h")).read()
    assert "st3r_param_activate_impl" in stages and "st3r_param_activate_bwd_impl" in stages
    assert os.path.exists(os.path.join(ROOT, "starst3r_amd", "csrc", "gs_activation.hip"))


def test_the_scene_has_the_two_settings_and_the_method():
    import starst3r_amd as st
    from starst3r_amd import gs
    scene = st.Scene(device="cpu")
    assert scene.activations is False and scene.init_opacity == 0.1
    assert "activate_3dgs" in gs.__all__ and callable(st.Scene.activate_3dgs)
    assert list(inspect.signature(gs.activate_3dgs).parameters) == ["scene", "eps"]
    assert inspect.signature(gs.activate_3dgs).parameters["eps"].default == 1e-4
    assert list(inspect.signature(st.Scene.activate_3dgs).parameters) == ["self", "eps"]
    # the argument lists users program against are the parent's
    assert list(inspect.signature(gs.init_3dgs).parameters) == ["scene", "init_scale", "lr"]
    for word in ("scene.activations",):
        assert word in gs.run_3dgs_optim.__doc__ and word in gs.render_3dgs.__doc__ and word in gs.init_3dgs.__doc__


def test_init_3dgs_under_the_setting_stores_logs_and_logits(no_ops):
    raw = _points(_scene())
    raw.init_3dgs(init_scale=3e-3)
    assert torch.all(raw.gaussians["scales"] == np.float32(3e-3)) and torch.all(raw.gaussians["opacities"] == 1.0)
    del raw.activations                                               # absent counts as False
    raw.init_3dgs()
    assert torch.all(raw.gaussians["opacities"] == 1.0)
    for init_scale, p in ((3e-3, 0.1), (0.25, 0.5), (7.0, 0.999)):
        scene = _points(_scene())
        scene.activations, scene.init_opacity = True, p
        scene.init_3dgs(init_scale=init_scale)
        g = scene.gaussians
        assert g["scales"].dtype == torch.float32 and tuple(g["scales"].shape) == (37, 3) and tuple(g["opacities"].shape) == (37,)
        assert torch.all(g["scales"] == np.float32(math.log(init_scale)))
        assert torch.all(g["opacities"] == np.float32(math.log(p) - math.log1p(-p)))
        # everything else is as without
        for k in ("means", "quats", "sh0", "shN"):
            assert torch.equal(g[k], raw.gaussians[k]), k
        assert scene._gs_optim.m.numel() == 23 * 37 and scene.activations is True
    scene = _points(_scene())
    scene.activations = True                                          # init_opacity: gsplat's 0.1 by default
    scene.init_3dgs()
    assert torch.all(scene.gaussians["opacities"] == np.float32(math.log(0.1 / 0.9)))


BAD_INIT = {
    # name: (activations, init_opacity, init_scale, the word the message must hold)
    "activations_int": (1, 0.1, 3e-3, "activations"),
    "activations_text": ("yes", 0.1, 3e-3, "activations"),
    "activations_none": (None, 0.1, 3e-3, "activations"),
    "activations_float": (0.0, 0.1, 3e-3, "activations"),
    "opacity_zero": (True, 0.0, 3e-3, "init_opacity"),
    "opacity_one": (True, 1.0, 3e-3, "init_opacity"),
    "opacity_negative": (True, -0.1, 3e-3, "init_opacity"),
    "opacity_nan": (True, float("nan"), 3e-3, "init_opacity"),
    "opacity_text": (True, "0.1", 3e-3, "init_opacity"),
    "opacity_bool": (True, True, 3e-3, "init_opacity"),
    "scale_zero": (True, 0.1, 0.0, "init_scale"),
    "scale_negative": (True, 0.1, -3e-3, "init_scale"),
    "scale_nan": (True, 0.1, float("nan"), "init_scale"),
    "scale_inf": (True, 0.1, float("inf"), "init_scale"),
}


@pytest.mark.parametrize("kind", sorted(BAD_INIT))
def test_bad_values_raise_before_anything_is_allocated(no_ops, kind):
    scene = _scene()                                                  # no dense points: touching them would assert
    scene.activations, scene.init_opacity, init_scale, word = BAD_INIT[kind]
    before = dict(scene.gaussians)
    with pytest.raises(ValueError, match=word):
        scene.init_3dgs(init_scale=init_scale)
    assert scene.gaussians == before and not hasattr(scene, "_gs_optim")
    if word == "activations":                                         # the other readers of the setting
        from starst3r_amd import gs
        with pytest.raises(ValueError, match=word):
            gs.run_3dgs_optim(scene, 1)
        with pytest.raises(ValueError, match=word):
            gs.run_3dgs_optim(scene, 1, exposure_lr=1e-3)             # before the other options' side effects too
        assert not hasattr(scene, "exposures")
        with pytest.raises(ValueError, match=word):
            scene.render_3dgs(scene.w2c, scene.intrinsics, 8, 6)
        with pytest.raises(ValueError, match=word):
            scene.activate_3dgs()


def _raw_scene(n=300, seed=3):
    """a CPU scene as init_3dgs leaves it, raw scales (signs, zeros) and opacities (in and out of [0, 1]), non-zero moments"""
    scene = _points(_scene(), n, seed)
    scene.init_3dgs()
    gen = torch.Generator().manual_seed(seed + 1)
    g = scene.gaussians
    s = torch.rand((n, 3), generator=gen) * 0.05 + 1e-3
    s[::7] *= -1.0
    s[5, 1] = 0.0
    s[6, 2] = 1e-38
    o = torch.rand(n, generator=gen) * 0.9 + 0.05
    o[0], o[1], o[2], o[3], o[4] = -0.3, 0.0, 1.0, 1.6, 5e-5
    g["scales"].data.copy_(s); g["opacities"].data.copy_(o)
    st = scene._gs_optim
    st.m.copy_(torch.randn(23 * n, generator=gen)); st.v.copy_(torch.rand(23 * n, generator=gen))
    st.step = 17
    return scene


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
def test_activate_3dgs_converts_in_place(no_ops, eps):
    scene = _raw_scene()
    g, st = scene.gaussians, scene._gs_optim
    s0, o0 = g["scales"].detach().clone(), g["opacities"].detach().clone()
    kept = {k: g[k].detach().clone() for k in ("means", "quats", "sh0", "shN")}
    m0, v0 = st.m.clone(), st.v.clone()
    params = {k: g[k] for k in g}
    if eps == 1e-4:
        scene.activate_3dgs()
    else:
        scene.activate_3dgs(eps)
    assert scene.activations is True and all(g[k] is params[k] for k in g)          # in place
    # the values agree with float64: the nearest float32 of log(max(|s|, 1e-30)) and logit(clamp(o, eps, 1 - eps))
    s64 = np.log(np.maximum(np.abs(s0.numpy().astype(np.float64)), 1e-30))
    o64 = np.clip(o0.numpy().astype(np.float64), eps, 1.0 - eps)
    o64 = np.log(o64) - np.log1p(-o64)
    for got, ref in ((g["scales"], s64), (g["opacities"], o64)):
        got = got.detach().numpy()
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 0.5 * np.spacing(np.abs(ref).astype(np.float32)) * (1 + 1e-9))
    assert g["scales"][5, 1] == np.float32(math.log(1e-30)) and g["opacities"][1] == np.float32(math.log(eps) - math.log1p(-eps))
    # what the renderer sees again: |s| and the clamped o, to float32
    S, O = ac.activate_reference(g["scales"].detach().numpy(), g["opacities"].detach().numpy())
    live = np.abs(s0.numpy()) > 1e-30
    assert np.allclose(S[live], np.abs(s0.numpy())[live], rtol=1e-5, atol=0)      # (half an ulp of a log near -87)
    assert np.allclose(O, np.clip(o0.numpy(), eps, 1 - eps), rtol=0, atol=2e-7)
    # the moments of the two blocks are zeroed, the other three blocks and the step counter keep their bits
    n = 300
    for key, lo, hi in (("means", 0, 3), ("quats", 3, 7), ("scales", 7, 10), ("opacities", 10, 11), ("shN", 11, 23)):
        sl = slice(lo * n, hi * n)
        assert sl == st.block_slice(key)
        if key in ("scales", "opacities"):
            assert torch.all(st.m[sl] == 0) and torch.all(st.v[sl] == 0)
        else:
            assert torch.equal(st.m[sl].view(torch.int32), m0[sl].view(torch.int32))
            assert torch.equal(st.v[sl].view(torch.int32), v0[sl].view(torch.int32))
    assert st.step == 17
    for k in kept:
        assert torch.equal(g[k].detach(), kept[k])
    # a second call is refused, and changes nothing
    s1, o1 = g["scales"].detach().clone(), g["opacities"].detach().clone()
    with pytest.raises(ValueError, match="activations"):
        scene.activate_3dgs()
    assert torch.equal(g["scales"].detach(), s1) and torch.equal(g["opacities"].detach(), o1)
    for bad in (0.0, 0.5, -1e-4, float("nan")):
        fresh = _raw_scene()
        with pytest.raises(ValueError, match="eps"):
            fresh.activate_3dgs(bad)
        assert fresh.activations is False


def test_the_off_setting_builds_no_option_and_on_builds_one(no_ops):
    from starst3r_amd import gs
    scene = _scene()
    assert gs._Activations.when_on(scene, False) is None
    del scene.activations
    assert gs._Activations.when_on(scene, False) is None and gs._activations(scene) is False
    scene.activations = True
    o = gs._Activations.when_on(scene, True)
    assert isinstance(o, gs._Activations) and isinstance(o, gs._PerViewOption) and o.counter is None


def test_the_option_sets_and_clears_the_context_setting(monkeypatch):
    """registered like the per-view options, and cleared in the same `finally` whatever ends the block"""
    import types
    from starst3r_amd import gs, ops
    calls = []
    monkeypatch.setattr(ops, "set_activation", lambda ctx, on: calls.append(("activation", on)))
    monkeypatch.setattr(ops, "set_gt_moments", lambda ctx, gt, mom: calls.append(("moments", gt is not None)))
    monkeypatch.setattr(gs, "_gt_moments", lambda scene, ctx, gt: "moments")
    scene = _scene()
    scene.activations = True
    c = types.SimpleNamespace(scene=scene, ctx="ctx", gt="gt")
    with pytest.raises(RuntimeError, match="stop"):
        with gs._registered(c, [gs._Activations.when_on(scene, False)]):
            assert calls == [("moments", True), ("activation", True)]
            raise RuntimeError("stop")
    assert calls[2:] == [("moments", False), ("activation", False)]


def test_it_is_refused_under_the_multi_gpu_settings(no_ops, monkeypatch):
    from starst3r_amd import dist as sdist, gs
    scene = _scene()
    scene.activations = True
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="scene.activations"):
        gs.run_3dgs_optim(scene, 1)
    monkeypatch.setattr(sdist, "rank_world", lambda: (0, 1))
    monkeypatch.setenv("ST3R_MULTI_GPU", "gaussian-sharded")
    with pytest.raises(NotImplementedError, match="scene.activations"):
        gs.run_3dgs_optim(scene, 1)
    with pytest.raises(NotImplementedError, match="scene.activations"):
        gs.run_3dgs_optim(scene, 1, enable_pruning=True)
    with pytest.raises(NotImplementedError, match="scene.activations"):
        gs._run_3dgs_optim_sharded(scene, 1, 0.2, 0.01, 0.01, False)   # a direct call of the sharded loop


def test_the_references_agree_with_autograd_and_with_each_other():
    """activation_cases: the float32 restatement of the backward is the float64 chain rule to a few roundings, the float64
    chain rule is torch autograd's, and the planted logits saturate without a NaN"""
    c = ac.kernel_inputs(257)
    S64, O64 = ac.activate_reference(c["s"], c["o"])
    S, O = ac.float32_of(S64), ac.float32_of(O64)
    assert ac.planted(c["o"]).sum() == 2 and np.all(np.isfinite(S)) and np.all(np.isfinite(O))
    assert O[-1] == 1.0 and 0.0 <= O[128] < 1e-38
    v_s, v_o = ac.activate_bwd_f32(S, O, c["v_S"], c["v_O"], c["k_s"], c["k_o"])
    r_s, r_o = ac.activate_bwd_reference(S, O, c["v_S"], c["v_O"], c["k_s"], c["k_o"])
    assert v_s.dtype == np.float32 and np.all(np.isfinite(v_s)) and np.all(np.isfinite(v_o)) and v_o[-1] == 0.0
    assert np.allclose(v_s, r_s, rtol=3e-7, atol=1e-44) and np.allclose(v_o, r_o, rtol=4e-7, atol=1e-44)
    s = torch.tensor(c["s"], dtype=torch.float64, requires_grad=True)
    o = torch.tensor(c["o"], dtype=torch.float64, requires_grad=True)
    k_s, k_o = float(c["k_s"]), float(c["k_o"])
    f = (torch.exp(s) * torch.tensor(c["v_S"], dtype=torch.float64)).sum() + k_s * torch.exp(s).sum() + \
        (torch.sigmoid(o) * torch.tensor(c["v_O"], dtype=torch.float64)).sum() + k_o * torch.sigmoid(o).sum()
    f.backward()
    a_s, a_o = ac.activate_bwd_reference(S64, O64, c["v_S"], c["v_O"], k_s, k_o)
    assert np.allclose(s.grad.numpy(), a_s, rtol=1e-9, atol=1e-12) and np.allclose(o.grad.numpy(), a_o, rtol=1e-9, atol=1e-300)
    # the sizes name the code's thresholds
    assert ac.stream_blocks(ac.N_TWO_TRIPS - 1) == 256 and ac.stream_blocks(ac.N_TWO_TRIPS) == 257
    assert ac.stream_blocks(ac.N_RAGGED) == 4 and ac.N_RAGGED % 4 == 3
    k = ac.reg_constants(3, 400, 0.01, 0.01)
    assert k[0].dtype == np.float32 and abs(float(k[0]) - 3 * 0.01 / 1200) < 1e-11 and abs(float(k[1]) - 3 * 0.01 / 400) < 1e-11
