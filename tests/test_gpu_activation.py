"""GPU tests of the activated parameterisation (scene.activations): the two streaming kernels of csrc/gs_activation.hip
through st3r_param_activate / st3r_param_activate_bwd, the context setting st3r_ctx_set_activation in the fused training
calls and st3r_gs_render, render_3dgs / init_3dgs / activate_3dgs / run_3dgs_optim under the scene setting.

    1. the kernels against tests/activation_cases.py            5. against float64, end to end
    2. the fused step equals the unfused chain, bit for bit      6. capability: relocation, training
    3. nothing else moves                                        7. a communicator
    4. the two parameterisations agree

The bars.  Forward kernel: MAX_ULP_S and MAX_ULP_O below are the largest errors measured on the inputs of
activation_cases.kernel_inputs over KERNEL_SIZES, rounded up to the next whole float32 ulp ("Activated scales
and opacities", holds the measured figures); they are compared wherever the float64 value lies in float32's normal range.
The planted logits -90 and +90 lie outside it on one side (sigmoid(-90) = 8e-40 is a float32 denormal, where an ulp is no
relative measure): there the assertion is the saturation itself, exactly 0 and exactly 1, and exact zeros in the gradient.
Backward kernel: the bits of activation_cases.activate_bwd_f32.  Sums: 1e-12 relative of the double sums of the stored
values.  Fused step: the bits of the unfused chain.  End to end: at most twice the error of the raw path, measured in the
same test against the same float64 renderer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import activation_cases as ac
from per_view_cases import (B1, B2, EPS, _Run, _optim_scene, _same_bits, _synthetic_prior, dev, make, masked_cotangents,
                            rel_err_per_camera)
from st3r_synth import synth

MAX_ULP_S = 1.0      # expf: 0.821 ulp measured (N = 262145)
MAX_ULP_O = 3.0      # 1 / (1 + expf(-o)): 2.218 ulp measured (N = 262145) -- expf's error, one add, one divide
SSIM_FAC, OPAC_FAC, SCALE_FAC = 0.2, 0.01, 0.01
DEPTH_FAC, ALPHA_FAC = 0.5, 0.5


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _placed(a, how):
    """the array on the device: "plain", or "shifted": a view that starts one float into a buffer"""
    a = np.ascontiguousarray(a, np.float32)
    if how == "plain":
        return dev(a)
    buf = torch.full((a.size + 1,), 7.0, device="cuda:0")
    view = buf[1:].view(a.shape)
    view.copy_(dev(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------
PLACEMENTS = [(n, "plain") for n in ac.KERNEL_SIZES] + [(n, "shifted") for n in (1, 5, 257, ac.N_RAGGED)]


@pytest.mark.parametrize("n,how", PLACEMENTS, ids=lambda p: str(p))
def test_kernels_against_the_references(ctx, n, how):
    from starst3r_amd import ops
    c = ac.kernel_inputs(n)
    s, o = _placed(c["s"], how), _placed(c["o"], how)
    out_s = _placed(np.full((n, 3), 7.0), how); out_o = _placed(np.full(n, 7.0), how)
    S, O, sums = ops.param_activate(ctx, s, o, out_s, out_o, want_sums=True)
    torch.cuda.synchronize()
    assert S is out_s and O is out_o
    S_h, O_h = S.cpu().numpy(), O.cpu().numpy()
    assert np.all(np.isfinite(S_h)) and np.all(np.isfinite(O_h))
    # forward: float32 ulps of the float64 value; the planted logits saturate to exactly 0 and 1
    S64, O64 = ac.activate_reference(c["s"], c["o"])
    live = ~ac.planted(c["o"])
    e_s = float(ac.ulp_error(S_h, S64).max())
    e_o = float(ac.ulp_error(O_h[live], O64[live]).max()) if live.any() else 0.0
    print("n = %d %s: exp max %.3f ulp, sigmoid max %.3f ulp" % (n, how, e_s, e_o))
    assert e_s <= MAX_ULP_S and e_o <= MAX_ULP_O
    assert np.all(O_h[c["o"] == 90.0] == 1.0) and np.all(O_h[c["o"] == -90.0] == 0.0)
    assert np.all((O_h >= 0.0) & (O_h <= 1.0)) and np.all(S_h > 0.0)
    # the two sums: of the stored float32 values, in double
    got = sums.cpu().numpy()
    want = np.array([O_h.astype(np.float64).sum(), S_h.astype(np.float64).sum()])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    # two runs, and a run without the sums: identical bits
    S2, O2, sums2 = ops.param_activate(ctx, s, o, want_sums=True)
    S3, O3, none = ops.param_activate(ctx, s, o)
    torch.cuda.synchronize()
    assert none is None and _same_bits(sums2.view(torch.float32), sums.view(torch.float32))
    for a in (S2, S3):
        assert np.array_equal(_bits32(a.cpu().numpy()), _bits32(S_h))
    for a in (O2, O3):
        assert np.array_equal(_bits32(a.cpu().numpy()), _bits32(O_h))
    # backward: the bits of the float32 restatement, with and without the regularisers' constants; in place = out of place
    for k_s, k_o in ((c["k_s"], c["k_o"]), (0.0, 0.0)):
        v_S, v_O = _placed(c["v_S"], how), _placed(c["v_O"], how)
        v_s, v_o = ops.param_activate_bwd(ctx, S, O, v_S, v_O, k_s, k_o)
        torch.cuda.synchronize()
        r_s, r_o = ac.activate_bwd_f32(S_h, O_h, c["v_S"], c["v_O"], k_s, k_o)
        g_s, g_o = v_s.cpu().numpy(), v_o.cpu().numpy()
        assert np.all(np.isfinite(g_s)) and np.all(np.isfinite(g_o))
        assert np.array_equal(_bits32(g_s), _bits32(r_s)) and np.array_equal(_bits32(g_o), _bits32(r_o))
        assert np.all(g_o[ac.planted(c["o"])] == 0.0)
        i_s, i_o = ops.param_activate_bwd(ctx, S, O, v_S, v_O, k_s, k_o, v_S, v_O)
        torch.cuda.synchronize()
        assert i_s is v_S and i_o is v_O
        assert np.array_equal(_bits32(v_S.cpu().numpy()), _bits32(g_s)) and np.array_equal(_bits32(v_O.cpu().numpy()), _bits32(g_o))
    if how == "shifted":   # the float in front of every output view was not touched
        for t in (out_s, out_o, v_S, v_O):
            assert t._base.numel() == t.numel() + 1 and float(t._base[0]) == 7.0


def test_the_bindings_check_their_tensors(ctx):
    from starst3r_amd import ops
    s, o = torch.zeros((5, 3), device="cuda:0"), torch.zeros(5, device="cuda:0")
    for bad_s, bad_o in ((s[:, :2], o), (s, o[:4]), (s.double(), o), (s, o.double()), (s.reshape(-1), o)):
        with pytest.raises(ValueError):
            ops.param_activate(ctx, bad_s, bad_o)
    with pytest.raises(ValueError):
        ops.param_activate(ctx, s, o, torch.zeros((4, 3), device="cuda:0"))
    with pytest.raises(ValueError):
        ops.param_activate_bwd(ctx, s, o, s, o[:4])
    with pytest.raises(ValueError):
        ops.param_activate_bwd(ctx, s, o, s.clone(), o.clone(), float("nan"), 0.0)
    assert ops.get_activation(ctx) is False
    assert ops.set_activation(ctx, True) is False and ops.get_activation(ctx) is True
    assert ops.set_activation(ctx, False) is True and ops.get_activation(ctx) is False


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused step equals the unfused chain
# ---------------------------------------------------------------------------------------------------------------------
def _activated_gaussians(N, V, W, H, seed):
    """a synthetic scene whose scales are logs and whose opacities are logits (opacities in [0.05, 0.95])"""
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=0.02, scale_hi=0.12)
    o = np.clip(g["opacities"].astype(np.float64), 0.05, 0.95)
    g = dict(g, scales=np.log(g["scales"].astype(np.float64)).astype(np.float32),
             opacities=(np.log(o) - np.log1p(-o)).astype(np.float32))
    return g, w2c, Ks


def _setup_activated(ctx, N=300, V=3, W=64, H=48, seed=7):
    """device parameters (logs, logits), cameras, and a noisy ground truth of the scene's own activated render"""
    from starst3r_amd import ops
    g, w2c, Ks = _activated_gaussians(N, V, W, H, seed)
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    S, O, _ = ops.param_activate(ctx, P["scales"], P["opacities"])
    PA = dict(P, scales=S, opacities=O)
    rgb, _, _ = ops.render(ctx, PA, vm, K, campos, W, H)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    gt = torch.clamp(rgb + 0.05 * torch.randn(rgb.shape, device="cuda:0", generator=gen), 0, 1).contiguous()
    return dict(g=g, w2c=w2c, Ks=Ks, P=P, PA=PA, vm=vm, K=K, campos=campos, gt=gt, W=W, H=H, N=N, V=V)


REGISTRATIONS = ("depth", "exposure", "intrinsics", "weights", "backgrounds", "alpha")


def _registration_tensors(ctx, R, which):
    """the payloads of the registrations named in `which`, from fixed seeds"""
    V, H, W = R["V"], R["H"], R["W"]
    gen = torch.Generator(device="cuda:0").manual_seed(33)
    T = {}
    if "depth" in which:
        T["depth"] = _synthetic_prior(ctx, R["PA"], R["vm"], R["K"], W, H)[:2]
    if "exposure" in which:
        T["exposure"] = (torch.eye(3, 4, device="cuda:0").repeat(V, 1, 1) +
                         0.1 * torch.randn((V, 3, 4), device="cuda:0", generator=gen)).contiguous()
    if "weights" in which:
        wt = 2.0 * torch.rand((V, H, W), device="cuda:0", generator=gen)
        wt[:, H // 4:H // 2, W // 3:2 * W // 3] = 0.0
        T["weights"] = wt.contiguous()
    if "backgrounds" in which:
        b = torch.rand((V, 3), device="cuda:0", generator=gen)
        b[0] = 1.0
        T["backgrounds"] = b.contiguous()
    if "alpha" in which:
        M = (torch.rand((V, H, W), device="cuda:0", generator=gen) > 0.5).float()
        w = 2.0 * torch.rand((V, H, W), device="cuda:0", generator=gen)
        w[-1, :H // 2] = 0.0
        T["alpha"] = (M.contiguous(), w.contiguous())
    return T


class _Registered:
    """the registrations of `which` with the ctx, with output buffers of this run (preset to 7: the step overwrites them)"""

    def __init__(self, ctx, R, which, T):
        self.ctx, self.R, self.which, self.T = ctx, R, which, T
        V = R["V"]
        self.vE = torch.full((V, 3, 4), 7.0, device="cuda:0") if "exposure" in which else None
        self.vK = torch.full((V, 4), 7.0, device="cuda:0") if "intrinsics" in which else None

    def __enter__(self):
        from starst3r_amd import ops
        ctx, gt, T = self.ctx, self.R["gt"], self.T
        if "depth" in self.which:
            ops.set_depth_prior(ctx, gt, T["depth"][0], T["depth"][1], DEPTH_FAC)
        if "exposure" in self.which:
            ops.set_exposure(ctx, gt, T["exposure"], self.vE)
        if "intrinsics" in self.which:
            ops.set_intrinsics_grad(ctx, gt, self.vK)
        if "weights" in self.which:
            ops.set_loss_weight(ctx, gt, T["weights"])
        if "backgrounds" in self.which:
            ops.set_background(ctx, gt, T["backgrounds"])
        if "alpha" in self.which:
            ops.set_alpha_target(ctx, gt, T["alpha"][0], T["alpha"][1], ALPHA_FAC)
        return self

    def __exit__(self, *exc):
        from starst3r_amd import ops
        ctx = self.ctx
        ops.set_depth_prior(ctx, None, None, None); ops.set_exposure(ctx, None, None, None)
        ops.set_intrinsics_grad(ctx, None, None); ops.set_loss_weight(ctx, None, None)
        ops.set_background(ctx, None, None); ops.set_alpha_target(ctx, None, None, None)
        ops.set_activation(ctx, False); ops.set_debug(ctx, 0)


def _run_steps(ctx, R, entry, fused, which=(), T=None, steps=5, debug=0, pose_lr=1e-4):
    """`steps` training steps from R's parameters through `entry` (fwd_bwd: train_fwd_bwd + adam_step; step: train_step;
    step_poses: train_step_poses).  fused: the ctx's activation is on and the calls get the logs and logits.  Not fused, the
    unfused chain: param_activate -> the same call with the activation off on the activated tensors with both regulariser
    factors 0 (for step / step_poses with the Gaussians' learning rate 0 and moments of its own, so that only the cameras
    move in it) -> param_activate_bwd in place on the gradient's blocks -> adam_step on the logs and logits.
    -> (run, snapshots per step of (grads, v_exposure, v_Ks, v_viewmats), composed float64 losses or None)"""
    from starst3r_amd import ops
    N, V, W, H, K, gt = R["N"], R["V"], R["W"], R["H"], R["K"], R["gt"]
    r = _Run(R["P"], R["vm"], R["campos"], steps)
    k_s, k_o = ac.reg_constants(V, N, OPAC_FAC, SCALE_FAC)
    snaps, composed = [], []
    with _Registered(ctx, R, which, T or {}) as reg:
        ops.set_debug(ctx, debug)
        for it in range(steps):
            loss = r.losses[it:it + 1]
            if fused:
                ops.set_activation(ctx, True)
                if entry == "fwd_bwd":
                    ops.train_fwd_bwd(ctx, r.P, r.vm, K, r.campos, gt, W, H, SSIM_FAC, OPAC_FAC, SCALE_FAC, r.grads, loss)
                    ops.adam_step(ctx, r.P, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, it + 1)
                elif entry == "step":
                    ops.train_step(ctx, r.P, r.vm, K, r.campos, gt, W, H, SSIM_FAC, OPAC_FAC, SCALE_FAC, r.grads, r.m, r.v,
                                   1e-3, B1, B2, EPS, it + 1, loss)
                else:
                    ops.train_step_poses(ctx, r.P, r.vm, K, r.campos, gt, W, H, SSIM_FAC, OPAC_FAC, SCALE_FAC, r.grads, r.m,
                                         r.v, 1e-3, B1, B2, EPS, it + 1, loss, r.pm, r.pv, pose_lr, it + 1, None, r.vvm)
            else:
                S, O, sums = ops.param_activate(ctx, r.P["scales"], r.P["opacities"], want_sums=True)
                PA = {k: v.clone() for k, v in r.P.items()}
                PA["scales"], PA["opacities"] = S.clone(), O.clone()
                if entry == "step_poses":
                    m0, v0 = torch.zeros_like(r.m), torch.zeros_like(r.v)
                    ops.train_step_poses(ctx, PA, r.vm, K, r.campos, gt, W, H, SSIM_FAC, 0.0, 0.0, r.grads, m0, v0, 0.0, B1, B2,
                                         EPS, it + 1, loss, r.pm, r.pv, pose_lr, it + 1, None, r.vvm)
                    assert _same_bits(PA["scales"], S) and _same_bits(PA["means"], r.P["means"])   # (rate 0 moved nothing)
                else:
                    ops.train_fwd_bwd(ctx, PA, r.vm, K, r.campos, gt, W, H, SSIM_FAC, 0.0, 0.0, r.grads, loss)
                G = ops.split_grads(r.grads, N)
                ops.param_activate_bwd(ctx, S, O, G["scales"], G["opacities"], k_s, k_o, G["scales"], G["opacities"])
                ops.adam_step(ctx, r.P, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, it + 1)
                torch.cuda.synchronize()
                composed.append(float(loss[0]) + ac.regularisers(S.cpu().numpy(), O.cpu().numpy(), V, OPAC_FAC, SCALE_FAC))
            snaps.append([r.grads.clone()] + [None if t is None else t.clone() for t in (reg.vE, reg.vK)] + [r.vvm.clone()])
        ops.settle(ctx)
    torch.cuda.synchronize()
    return r, snaps, composed


def _assert_same_run(tag, fused, unfused):
    (rf, sf, _), (ru, su, composed) = fused, unfused
    for it, (a, b) in enumerate(zip(sf, su)):
        for name, x, y in zip(("grads", "v_exposure", "v_Ks", "v_viewmats"), a, b):
            if x is not None:
                assert _same_bits(x, y), (tag, "step", it, name, float((x - y).abs().max()))
        assert float(a[0].abs().max()) > 0
    for x, y in zip(rf.state()[:-1], ru.state()[:-1]):   # parameters, moments, cameras and their moments
        assert _same_bits(x, y), tag
    lf = rf.losses.double().cpu().numpy()
    rel = np.abs(lf - np.array(composed)) / np.abs(np.array(composed))
    print(tag, "fused loss against its float64 composition: max rel %.2e" % rel.max())
    assert np.all(rel <= 1e-6), (tag, lf, composed)


@pytest.mark.parametrize("entry", ["fwd_bwd", "step", "step_poses"])
def test_fused_entry_points_equal_the_unfused_chain(ctx, entry):
    R = _setup_activated(ctx)
    fused, unfused = _run_steps(ctx, R, entry, True), _run_steps(ctx, R, entry, False)
    _assert_same_run(entry, fused, unfused)
    if entry == "step_poses":
        assert float(fused[1][0][3].abs().max()) > 0 and not _same_bits(fused[0].vm, R["vm"])   # the cameras moved
    from starst3r_amd import ops
    assert ops.get_activation(ctx) is False


def test_two_view_chunks(ctx):
    """debug flag 32: both sides walk the three views in chunks of one and two; the chain rule runs once, behind the last"""
    from starst3r_amd import ops
    c = ops.Context("cuda:0")   # a context of its own: the chunk count sticks to the context that walked in chunks
    R = _setup_activated(c)
    fused, unfused = _run_steps(c, R, "step", True, debug=32), _run_steps(c, R, "step", False, debug=32)
    c.close()
    _assert_same_run("two chunks", fused, unfused)
    whole = _run_steps(ctx, R, "step", True, steps=1)
    rel = float((whole[1][0][0] - fused[1][0][0]).abs().max() / whole[1][0][0].abs().max())
    print("two view chunks against one: grads max rel %.1e" % rel)
    assert rel < 1e-5


@pytest.mark.parametrize("which", [(w,) for w in REGISTRATIONS] + [REGISTRATIONS], ids=lambda w: "+".join(w))
def test_every_registration_alone_and_all_together(ctx, which):
    """the pose and intrinsics gradients of the fused step are those of the raw step on the activated tensors, which runs
    the stand-alone kernels (test_gpu_pose_train.py, test_gpu_intrinsics_train.py)"""
    R = _setup_activated(ctx)
    T = _registration_tensors(ctx, R, which)
    entry = "step_poses" if len(which) > 1 or which[0] in ("depth", "intrinsics") else "step"
    fused, unfused = _run_steps(ctx, R, entry, True, which, T), _run_steps(ctx, R, entry, False, which, T)
    _assert_same_run("+".join(which), fused, unfused)
    for buf in fused[1][0][1:3]:
        assert buf is None or not bool((buf == 7.0).any())
    none = _run_steps(ctx, R, entry, True, steps=1)
    assert not _same_bits(none[1][0][0], fused[1][0][0]) or which == ("intrinsics",)   # the registration does something


def test_an_overflowing_step_is_repeated(ctx):
    """debug flag 8 halves the capacity of an asynchronous step: Adam is skipped on the device, the activated copies are
    rebuilt by the repeated call, and the run ends with the bits of a run that never overflowed"""
    from starst3r_amd import _lib, ops

    def steps(overflow_at):
        c = ops.Context("cuda:0")
        R = _setup_activated(c, N=600, V=3, W=64, H=48, seed=9)
        r = _Run(R["P"], R["vm"], R["campos"], 3)
        ops.set_activation(c, True)
        it = 0
        while it < 3:
            before = [x.clone() for x in r.state()[:-1]] if it == overflow_at else None
            if it == overflow_at:
                ops.set_debug(c, 8)
            ops.train_step(c, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], SSIM_FAC, OPAC_FAC, SCALE_FAC, r.grads,
                           r.m, r.v, 1e-3, B1, B2, EPS, it + 1, r.losses[it:it + 1], want_stats=False)
            ops.set_debug(c, 0)
            if it == overflow_at:
                overflow_at = -1
                with pytest.raises(_lib.St3rError) as e:
                    ops.settle(c)
                assert e.value.code == -3
                for x, y in zip(r.state()[:-1], before):
                    assert _same_bits(x, y)
                continue
            it += 1
        ops.settle(c)
        torch.cuda.synchronize()
        c.close()
        return r
    a, b = steps(-1), steps(1)
    assert float(a.m.abs().max()) > 0
    for x, y in zip(a.state(), b.state()):
        assert _same_bits(x, y)


def test_st3r_gs_render_activates_under_the_setting(ctx):
    from starst3r_amd import ops
    R = _setup_activated(ctx)
    want = ops.render(ctx, R["PA"], R["vm"], R["K"], R["campos"], R["W"], R["H"])
    ops.set_activation(ctx, True)
    try:
        got = ops.render(ctx, R["P"], R["vm"], R["K"], R["campos"], R["W"], R["H"])
    finally:
        ops.set_activation(ctx, False)
    raw = ops.render(ctx, R["P"], R["vm"], R["K"], R["campos"], R["W"], R["H"])
    torch.cuda.synchronize()
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and not _same_bits(raw[0], want[0])


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
def _raw_scene_run(touch):
    """two raw train_steps with profiling, a render_3dgs with a backward and five iterations of run_3dgs_optim on a context
    of its own; touch(ctx) runs first"""
    from starst3r_amd import ops
    c = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P = {k: dev(v) for k, v in g.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(c, P, vm, K, campos, W, H)
    gt = rgb.clamp(0, 1).contiguous()
    touch(c)
    ops.set_profiling(c, True)
    r = _Run(P, vm, campos, 2)
    for it in range(2):
        ops.train_step(c, r.P, r.vm, K, r.campos, gt, W, H, 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3, B1, B2, EPS, it + 1,
                       r.losses[it:it + 1], want_stats=(it == 0))
    ops.settle(c)
    counts = {k: v[1] for k, v in ops.stage_ms(c).items()}
    ops.set_profiling(c, False)
    counts["arena_bytes"] = c.arena_bytes()
    torch.cuda.synchronize()
    out = r.state() + [r.grads]
    c.close()
    return out, counts


def test_with_the_setting_off_nothing_moves(ctx):
    from starst3r_amd import ops

    def set_then_clear(c):
        ops.set_activation(c, True)
        ops.set_activation(c, False)

    a, counts_a = _raw_scene_run(lambda c: None)
    b, counts_b = _raw_scene_run(set_then_clear)
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    # one sample per stage and step, as before, and no scratch of the activation
    assert counts_a == counts_b, (counts_a, counts_b)
    for stage in ("project", "scan", "emit", "sort", "offsets", "blend_fwd", "loss", "blend_bwd", "project_bwd", "adam",
                  "sort_depth"):
        assert counts_a[stage] == 2, (stage, counts_a)
    # render_3dgs and run_3dgs_optim: a scene without the attribute, one with False, one that was set and cleared
    g, w2c, Ks, W, H = make("small")
    imgs = np.full((w2c.shape[0], H, W, 3), 0.5, np.float32)
    outs = []
    for kind in ("absent", "false", "cleared"):
        scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
        if kind == "absent":
            del scene.activations
        elif kind == "cleared":
            ops.set_activation(ctx, True); ops.set_activation(ctx, False)
        img, alpha, info = scene.render_3dgs_original(W, H)
        (img.sum() + alpha.sum()).backward()
        grads = [scene.gaussians[k].grad.clone() for k in ("means", "quats", "scales", "opacities", "shN")]
        losses = scene.run_3dgs_optim(5)
        torch.cuda.synchronize()
        outs.append([img.detach(), alpha.detach(), info["opacities"]] + grads +
                    [scene.gaussians[k].data for k in sorted(scene.gaussians)] + [torch.tensor(losses)])
        assert ops.get_activation(ctx) is False
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert _same_bits(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two parameterisations agree
# ---------------------------------------------------------------------------------------------------------------------
MODES = ("RGB", "D", "ED", "RGB+D", "RGB+ED")
# The activated scene renders exp(log(s)) and sigmoid(logit(o)) in place of s and o: each is the raw value to a few float32
# roundings -- log(s) near -7 is stored to 2.4e-7, so exp of it is off by up to 2.4e-7 relative (four ulps of s), the
# logit's rounding moves o by up to 6e-8 |logit| o (1 - o) < 4e-8 -- a perturbation of the inputs of the size of the float32
# roundings inside the renderer, which the renderer's conditioning turns into the same kind of error.  The bars are those
# of section 5: twice the raw path's own error against float64 as measured there (DESIGN.md holds the figures), the
# forward's for the render and the worst gradient block's for the gradients; the modes with an expected depth have
# their own pair, measured on "RGB+ED", and follow the rule of tests/test_gpu_depth.py: the quotient D / alpha amplifies
# float32 noise where alpha is small, so ED is compared, and carries a cotangent, where alpha > 0.05.
EQUIV_BARS = {False: (2 * 5.92e-6, 2 * 1.0e-5), True: (2 * 5.92e-6, 2 * 8.1e-6)}   # expected depth in the mode: (render, gradients)


@pytest.mark.parametrize("name", ["small", "ragged", "wide"])
def test_the_activated_scene_renders_what_the_raw_scene_renders(name, oracle_built):
    from starst3r_amd import ops
    g, w2c, Ks, W, H = make(name)
    rng = np.random.default_rng(5)
    N = g["means"].shape[0]
    g = dict(g, opacities=rng.uniform(0.05, 0.95, N).astype(np.float32),
             scales=np.exp(rng.uniform(np.log(1e-3), np.log(5e-2), (N, 3))).astype(np.float32))
    v_rgb, v_alpha = masked_cotangents(g, w2c, Ks, W, H)
    v_depth = np.where(v_alpha != 0, rng.standard_normal(v_alpha.shape), 0.0).astype(np.float32)
    imgs = np.zeros((w2c.shape[0], H, W, 3), np.float32)
    scene = _optim_scene(g, torch.tensor(w2c), Ks, imgs)
    keys = ("means", "quats", "scales", "opacities", "shN")
    thick = scene.render_3dgs_original(W, H)[1].detach() > 0.05          # [V,H,W,1]: where an expected depth means something

    def render(mode):
        for k in keys:
            scene.gaussians[k].grad = None
        img, alpha, info = scene.render_3dgs_original(W, H, render_mode=mode)
        v_d = dev(v_depth) * thick if mode.endswith("ED") else dev(v_depth)
        cot = dev(v_rgb) if mode == "RGB" else (v_d if not mode.startswith("RGB") else torch.cat([dev(v_rgb), v_d], dim=-1))
        ((img * cot).sum() + (alpha * dev(v_alpha)).sum()).backward()
        torch.cuda.synchronize()
        img = img.detach().clone()
        if mode.endswith("ED"):
            img[..., -1:] = img[..., -1:] * thick
        return img, alpha.detach(), {k: scene.gaussians[k].grad.clone() for k in keys}, info

    raw = {m: render(m) for m in MODES}
    scene.activate_3dgs()
    S, O, _ = ops.param_activate(ops.get_context("cuda:0"), scene.gaussians["scales"].data, scene.gaussians["opacities"].data)
    for m in MODES:
        img, alpha, G, info = render(m)
        img_r, alpha_r, G_r, _ = raw[m]
        assert bool(torch.isfinite(img).all()) and _same_bits(info["opacities"], O[info["gaussian_ids"].long()])
        e_img = max(rel_err_per_camera(img, img_r) + rel_err_per_camera(alpha, alpha_r))
        # the gradients with respect to the raw tensors are recovered by dividing by S and by O (1 - O)
        G = dict(G, scales=G["scales"] / S, opacities=G["opacities"] / (O * (1 - O)))
        e_grad = {k: float((G[k] - G_r[k]).abs().max() / G_r[k].abs().max()) for k in keys if float(G_r[k].abs().max()) > 0}
        print(name, m, "activated against raw: render %.2e, gradients %s" % (e_img, {k: "%.1e" % e for k, e in e_grad.items()}))
        bar_img, bar_grad = EQUIV_BARS[m.endswith("ED")]
        assert e_img <= bar_img, (name, m, e_img)
        assert max(e_grad.values()) <= bar_grad, (name, m, e_grad)


# ---------------------------------------------------------------------------------------------------------------------
# 5. against float64, end to end
# ---------------------------------------------------------------------------------------------------------------------
def _block_errors(G, ref):
    return {k: float(np.abs(np.asarray(G[k], np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in ref}


def _split(grads, N):
    from starst3r_amd import ops
    return {k: v.double().cpu().numpy() for k, v in ops.split_grads(grads, N).items()}


def test_against_float64_end_to_end(ctx, oracle_built):
    """render_3dgs forward, its autograd gradients and one train_fwd_bwd with both regularisers, activated, against
    activation_cases.dense_render / dense_step; next to each the raw path on float32(exp(s)), float32(sigmoid(o)) computed in
    float64, against the same float64 renderer: the activated path may err at most twice as much."""
    from starst3r_amd import ops
    N, V, W, H = 300, 3, 64, 48
    g, w2c, Ks = _activated_gaussians(N, V, W, H, 7)
    S32, O32 = ac.activated_inputs_f32(g["scales"], g["opacities"])
    g_raw = dict(g, scales=S32, opacities=O32)
    vis, rad, margin = ac.visibility(g, w2c, Ks, W, H, S32, O32)
    ok = margin > 1e-4
    rng = np.random.default_rng(3)
    v_rgb = np.where(ok.reshape(V, H, W, 1), rng.standard_normal((V, H, W, 3)), 0.0).astype(np.float32)
    v_alpha = np.where(ok.reshape(V, H, W, 1), rng.standard_normal((V, H, W, 1)), 0.0).astype(np.float32)
    okt = torch.tensor(ok.reshape(V, H, W, 1))
    keys = ("means", "quats", "scales", "opacities", "shN")
    imgs = np.zeros((V, H, W, 3), np.float32)
    from test_gpu_depth import render_dense_depth   # (gs_torch_ref.render_dense with the depth of the same weights)
    v_ed = np.where(ok.reshape(V, H, W, 1), rng.standard_normal((V, H, W, 1)), 0.0).astype(np.float32)
    zero = torch.zeros(1, dtype=torch.float64)
    print("pixels float32 does not determine: %d of %d" % (int((~ok).sum()), ok.size))
    for mode in ("RGB", "RGB+ED"):
        errs, thick = {}, None
        for kind, gg, activated in (("raw", g_raw, False), ("activated", g, True)):
            rgb_t, alpha_t, d_t, P64 = ac.dense_render(gg, w2c, Ks, W, H, vis, rad, activated, render_dense_depth)
            if thick is None:   # an expected depth is compared, and carries a cotangent, where alpha > 0.05 (test_gpu_depth.py)
                thick = (alpha_t.detach() > 0.05) & okt
            img_t, cot = rgb_t, v_rgb
            if mode == "RGB+ED":
                img_t = torch.cat([rgb_t, d_t / alpha_t.clamp(min=1e-10)], dim=-1)
                cot = np.concatenate([v_rgb, v_ed * thick.numpy()], axis=-1)
            ((img_t * torch.tensor(cot, dtype=torch.float64)).sum() +
             (alpha_t * torch.tensor(v_alpha, dtype=torch.float64)).sum()).backward()
            ref = {k: P64[k].grad.numpy() for k in keys}
            ref["shN"] = ref["shN"][:, :4]
            scene = _optim_scene(gg, torch.tensor(w2c), Ks, imgs)
            scene.activations = activated
            img, alpha, _ = scene.render_3dgs_original(W, H, render_mode=mode)
            ((img * dev(cot)).sum() + (alpha * dev(v_alpha)).sum()).backward()
            torch.cuda.synchronize()
            G = {k: scene.gaussians[k].grad.double().cpu().numpy() for k in keys}
            G["shN"] = G["shN"][:, :4]
            seen = okt.expand(V, H, W, 3) if mode == "RGB" else torch.cat([okt.expand(V, H, W, 3), thick], dim=-1)
            e_fwd = max(rel_err_per_camera(torch.where(seen, img.detach().double().cpu(), zero),
                                           torch.where(seen, img_t.detach(), zero)) +
                        rel_err_per_camera(torch.where(okt, alpha.detach().double().cpu(), zero),
                                           torch.where(okt, alpha_t.detach(), zero)))
            errs[kind] = (e_fwd, _block_errors(G, ref))
            print("render_3dgs %s %s against float64: forward %.2e, gradients %s"
                  % (mode, kind, e_fwd, {k: "%.1e" % e for k, e in errs[kind][1].items()}))
        assert errs["activated"][0] <= 2 * errs["raw"][0], (mode, errs)
        for k in errs["raw"][1]:
            assert errs["activated"][1][k] <= 2 * errs["raw"][1][k], (mode, k, errs)
    # one training call with both regularisers on
    P = {k: dev(v) for k, v in g.items()}
    PR = {k: dev(v) for k, v in g_raw.items()}
    vm, K = dev(w2c), dev(Ks)
    campos = ops.camera_positions(vm)
    rgb, _, _ = ops.render(ctx, PR, vm, K, campos, W, H)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    gt = torch.clamp(rgb + 0.05 * torch.randn(rgb.shape, device="cuda:0", generator=gen), 0, 1).contiguous()
    gt_h = gt.cpu().numpy()
    step = {}
    for kind, Pd, gg, activated in (("raw", PR, g_raw, False), ("activated", P, g, True)):
        grads = torch.empty(23 * N, device="cuda:0"); loss = torch.zeros(1, device="cuda:0")
        ops.set_activation(ctx, activated)
        try:
            ops.train_fwd_bwd(ctx, Pd, vm, K, campos, gt, W, H, SSIM_FAC, OPAC_FAC, SCALE_FAC, grads, loss)
        finally:
            ops.set_activation(ctx, False)
        torch.cuda.synchronize()
        if activated:
            loss64, ref = ac.dense_step(gg, w2c, Ks, W, H, gt_h, vis, rad, SSIM_FAC, OPAC_FAC, SCALE_FAC)
        else:   # the raw path's own float64 statement: view_loss on the raw tensors (tests/test_gpu_psnr.py)
            from oracle import gs_torch_ref as tr
            rgb_t, _, P64 = ac.dense_render(gg, w2c, Ks, W, H, vis, rad, False)
            GT = torch.tensor(gt_h, dtype=torch.float64)
            l = sum(tr.view_loss(rgb_t[c], GT[c], P64["opacities"], P64["scales"], float(np.float32(SSIM_FAC)),
                                 float(np.float32(OPAC_FAC)), float(np.float32(SCALE_FAC))) for c in range(V))
            l.backward()
            loss64 = float(l.detach())
            ref = {k: P64[k].grad.numpy() for k in ("means", "quats", "scales", "opacities")}
            ref["sh"] = P64["shN"].grad.numpy()[:, :4]
        step[kind] = (abs(float(loss[0]) - loss64) / abs(loss64), _block_errors(_split(grads, N), ref))
        print("train_fwd_bwd %s against float64: loss %.2e, gradients %s"
              % (kind, step[kind][0], {k: "%.1e" % e for k, e in step[kind][1].items()}))
    assert step["activated"][0] <= max(2 * step["raw"][0], 2 * 2.0 ** -24), step   # (not below one float32 rounding of the loss)
    for k in step["raw"][1]:
        assert step["activated"][1][k] <= 2 * step["raw"][1][k], (k, step)


# ---------------------------------------------------------------------------------------------------------------------
# 6. capability
# ---------------------------------------------------------------------------------------------------------------------
def _capability_scene(activated=True, seed=11):
    """three 64 x 48 views: photographs of a synthetic scene, Gaussians initialised by init_3dgs from its jittered means"""
    import starst3r_amd as st
    from starst3r_amd import ops
    N, V, W, H = 400, 3, 64, 48
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=0.03, scale_hi=0.1)
    c = ops.get_context("cuda:0")
    vm, K = dev(w2c), dev(Ks)
    photos, _, _ = ops.render(c, {k: dev(v) for k, v in g.items()}, vm, K, ops.camera_positions(vm), W, H)
    photos = photos.clamp(0, 1).cpu().numpy()
    scene = st.Scene(device="cuda:0")
    scene.imgs = [photos[i] for i in range(V)]
    scene.c2w = torch.inverse(torch.tensor(w2c).double()).float()
    scene.intrinsics = torch.tensor(Ks)
    rng = np.random.default_rng(seed)
    scene.dense_pts = [torch.tensor(g["means"] + rng.normal(0, 0.01, g["means"].shape).astype(np.float32))]
    scene.dense_cols = [torch.tensor(rng.uniform(0, 1, (N, 3)).astype(np.float32))]
    scene.activations = activated
    scene.init_3dgs(init_scale=0.05)
    return scene, W, H


def test_relocation_acts_on_what_is_rendered():
    scene, W, H = _capability_scene()
    g = scene.gaussians
    N = g["means"].shape[0]
    dead = torch.arange(0, N, 10, device="cuda:0")
    g["opacities"].data[dead] = -8.0
    scene.strategy.step_post_backward(g, scene.optimizers, scene.strategy_state, step=600, info=None, lr=1e-3)
    torch.cuda.synchronize()
    g = scene.gaussians
    assert scene.strategy_state["n_relocated"] == dead.numel() == N // 10
    assert g["means"].shape[0] == N + scene.strategy_state["n_added"] and scene.strategy_state["n_added"] == int(0.05 * N)
    O = torch.sigmoid(g["opacities"].data.double())
    print("after relocation: min sigmoid(o) %.5f of %d Gaussians" % (float(O.min()), O.numel()))
    assert float(O.min()) >= scene.strategy.min_opacity * (1 - 1e-6)     # (the logit of min_opacity is stored in float32)
    assert all(bool(torch.isfinite(g[k].data).all()) for k in g)
    img, alpha, info = scene.render_3dgs_original(W, H)
    assert bool(torch.isfinite(img).all()) and float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    assert float(info["opacities"].min()) > 0.0 and float(info["opacities"].max()) < 1.0


def _psnr(scene, W, H):
    img, _, _ = scene.render_3dgs_original(W, H)
    gt = torch.tensor(np.stack(scene.imgs), device="cuda:0")
    return float(-10.0 * torch.log10(((img.detach() - gt) ** 2).mean()))


def test_training_on_logs_and_logits():
    from starst3r_amd import gs, ops
    iters = 100
    scene, W, H = _capability_scene()
    twin, _, _ = _capability_scene()
    losses = scene.run_3dgs_optim(iters)
    torch.cuda.synchronize()
    c = ops.get_context("cuda:0")
    assert ops.get_activation(c) is False                              # the setting belongs to the call
    assert len(losses) == iters and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert all(bool(torch.isfinite(scene.gaussians[k].data).all()) for k in scene.gaussians)
    # the same run step by step through ops
    g, st = twin.gaussians, twin._gs_optim
    views = list(range(len(twin.imgs)))
    gt = gs._gt_on_device(twin, views)
    vm = twin.w2c.to("cuda:0", torch.float32)[views].contiguous()
    K = twin.intrinsics.to("cuda:0", torch.float32)[views].contiguous()
    campos = ops.camera_positions(vm)
    P = {k: g[k].data for k in ("means", "quats", "scales", "opacities")}
    P["shN"] = g["shN"].data[:, :4].contiguous()
    out = torch.zeros(iters, device="cuda:0")
    ops.set_gt_moments(c, gt, ops.gt_moments(c, gt))
    ops.set_activation(c, True)
    try:
        for it in range(iters):
            ops.train_step(c, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, st.grads, st.m, st.v, st.lr, st.betas[0],
                           st.betas[1], st.eps, it + 1, out[it:it + 1], want_stats=False)
        ops.settle(c)
    finally:
        ops.set_activation(c, False)
        ops.set_gt_moments(c, None, None)
    torch.cuda.synchronize()
    assert float(np.float32(losses[-1])) == float(out[-1]) and np.array_equal(np.array(losses, np.float32), out.cpu().numpy())
    for k in ("means", "quats", "scales", "opacities"):
        assert _same_bits(scene.gaussians[k].data, P[k]), k
    # recorded, not asserted: the PSNR against a raw-mode run of the same length
    raw, _, _ = _capability_scene(activated=False)
    raw.run_3dgs_optim(iters)
    print("PSNR after %d iterations: activated %.2f dB, raw %.2f dB; activated loss %.5f -> %.5f"
          % (iters, _psnr(scene, W, H), _psnr(raw, W, H), losses[0], losses[-1]))


def test_run_3dgs_optim_with_every_option_and_pruning():
    """the setting composes with enable_pruning and with the per-view options, and a raw scene converted by activate_3dgs
    trains on"""
    scene, W, H = _capability_scene(activated=False)
    V = len(scene.imgs)
    first = scene.run_3dgs_optim(10)
    scene.activate_3dgs()
    after = scene.run_3dgs_optim(10, enable_pruning=True)
    assert all(np.isfinite(first)) and all(np.isfinite(after))
    scene.depth_maps = [torch.full((H, W), 3.0) for _ in range(V)]
    scene.intrinsics_lr, scene.intrinsics_freeze = 1e-4, (0,)
    scene.loss_masks = [np.ones((H, W), np.float32) for _ in range(V)]
    scene.backgrounds = np.zeros((V, 3), np.float32)
    scene.alpha_fac, scene.alpha_masks = 0.1, [np.ones((H, W), np.float32) for _ in range(V)]
    mix = scene.run_3dgs_optim(10, enable_pruning=True, pose_lr=1e-4, pose_freeze=(0,), depth_fac=0.1, exposure_lr=1e-3,
                               exposure_freeze=(0,))
    torch.cuda.synchronize()
    assert len(mix) == 10 and all(np.isfinite(mix))
    assert all(bool(torch.isfinite(scene.gaussians[k].data).all()) for k in scene.gaussians)


def test_the_example_of_activated_training():
    """examples/activated_training.py in small: raw training, activate_3dgs, then training with enable_pruning past the
    first refinement step -- it relocates the Gaussians whose rendered opacity is dead"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(__file__)), "examples", "activated_training.py")
    spec = importlib.util.spec_from_file_location("activated_training", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    out = mod.main(views=3, iters_raw=50, iters_pruned=601, W=128, H=96)
    print("example:", out)
    assert np.isfinite(out["loss_raw"]) and np.isfinite(out["loss_activated"])
    assert out["n_refinements"] == 1 and out["n_relocated"] >= 0
    assert out["min_rendered_opacity"] >= 0.0 and out["max_rendered_opacity"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 7. a communicator
# ---------------------------------------------------------------------------------------------------------------------
def test_the_setting_with_a_communicator_is_invalid():
    from starst3r_amd import dist as sdist, ops
    c = ops.Context("cuda:0")
    R = _setup_activated(c)
    r = _Run(R["P"], R["vm"], R["campos"], 1)
    r.grads.fill_(7.0)
    before = [x.clone() for x in r.state() + [r.grads]]
    sdist.attach_native_comm(c)
    ops.set_activation(c, True)
    try:
        with pytest.raises(ValueError, match="communicator"):
            ops.train_fwd_bwd(c, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.01, 0.01, r.grads, r.losses[0:1])
        with pytest.raises(ValueError, match="communicator"):
            ops.train_step(c, r.P, r.vm, R["K"], r.campos, R["gt"], R["W"], R["H"], 0.2, 0.01, 0.01, r.grads, r.m, r.v, 1e-3,
                           B1, B2, EPS, 1, r.losses[0:1])
        with pytest.raises(NotImplementedError, match="activat"):
            sdist.ShardedTrainer(c, r.P, R["N"], R["vm"], R["K"], R["gt"], R["W"], R["H"], 0, 1)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(r.state() + [r.grads], before))
    finally:
        ops.set_activation(c, False)
        sdist.detach_native_comm(c)
        c.close()
