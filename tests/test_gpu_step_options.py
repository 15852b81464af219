"""The options of the fused training step under a communicator: view-sharded training takes none of the eight -- the six
registrations (depth prior, exposures, intrinsics gradient, loss weights, backgrounds, alpha targets), an SH degree other
than (1, 1) and the activation -- and one table in st3r_train_fwd_bwd_impl (csrc/fused_step.hip) refuses them all, before
anything of the caller's is written.  Run on the MI355X box:
    python -m pytest tests/test_gpu_step_options.py -m gpu -q -s
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from per_view_cases import B1, B2, EPS, _same_bits, _setup, make


def _option(ops, ctx, name, gt, vE, vK):
    """sets the option on ctx -> (the call that clears it, as the refusal must name it; the function that clears it)"""
    V, H, W = gt.shape[:3]
    gen = torch.Generator().manual_seed(5)
    maps = [torch.rand((V, H, W), generator=gen).cuda() for _ in range(2)]
    if name == "depth_prior":
        ops.set_depth_prior(ctx, gt, 1.0 + maps[0], maps[1], 0.5)
        return "st3r_ctx_set_depth_prior", lambda: ops.set_depth_prior(ctx, None, None, None)
    if name == "exposure":
        ops.set_exposure(ctx, gt, torch.eye(3, 4, device="cuda:0").repeat(V, 1, 1), vE)
        return "st3r_ctx_set_exposure", lambda: ops.set_exposure(ctx, None, None, None)
    if name == "intrinsics_grad":
        ops.set_intrinsics_grad(ctx, gt, vK)
        return "st3r_ctx_set_intrinsics_grad", lambda: ops.set_intrinsics_grad(ctx, None, None)
    if name == "loss_weight":
        ops.set_loss_weight(ctx, gt, maps[0])
        return "st3r_ctx_set_loss_weight", lambda: ops.set_loss_weight(ctx, None, None)
    if name == "background":
        ops.set_background(ctx, gt, torch.rand((V, 3), generator=gen).cuda())
        return "st3r_ctx_set_background", lambda: ops.set_background(ctx, None, None)
    if name == "alpha_target":
        ops.set_alpha_target(ctx, gt, maps[0], maps[1], 0.5)
        return "st3r_ctx_set_alpha_target", lambda: ops.set_alpha_target(ctx, None, None, None)
    if name == "sh_degree":
        prev = ops.set_sh_degree(ctx, 0, 0, None)
        return "st3r_ctx_set_sh_degree", lambda: ops.set_sh_degree(ctx, *prev)
    assert name == "activation"
    ops.set_activation(ctx, True)
    return "st3r_ctx_set_activation", lambda: ops.set_activation(ctx, False)


@pytest.mark.parametrize("name", ["depth_prior", "exposure", "intrinsics_grad", "loss_weight", "background", "alpha_target",
                                  "sh_degree", "activation"])
def test_an_option_with_a_communicator_is_invalid(name):
    """train_fwd_bwd and train_step on a context with a one-rank communicator and the option set: ST3R_ERR_INVALID
    (ValueError) with a message that says "communicator" and names the call that clears the option, and every buffer of
    the caller -- parameters, grads, moments, loss slot, v_exposure, v_Ks, all pre-filled -- keeps its bits"""
    from starst3r_amd import dist as sdist, ops
    ctx = ops.Context("cuda:0")
    g, w2c, Ks, W, H = make("small")
    P, vm, K, campos, gt = _setup(ctx, g, w2c, Ks, W, H)
    N, V = P["means"].shape[0], vm.shape[0]
    grads = torch.full((23 * N,), 7.0, device="cuda:0")
    m, v = torch.full_like(grads, 0.25), torch.full_like(grads, 0.5)
    loss = torch.full((1,), 7.0, device="cuda:0")
    vE, vK = torch.full((V, 3, 4), 7.0, device="cuda:0"), torch.full((V, 4), 7.0, device="cuda:0")
    buffers = [P[k] for k in sorted(P)] + [grads, m, v, loss, vE, vK, vm, campos]
    before = [x.clone() for x in buffers]
    sdist.attach_native_comm(ctx)
    clearing_call, clear = _option(ops, ctx, name, gt, vE, vK)
    try:
        with pytest.raises(ValueError, match="communicator") as e:   # ST3R_ERR_INVALID (_lib.check)
            ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, loss)
        assert clearing_call + "(" in str(e.value)
        with pytest.raises(ValueError, match="communicator") as e:
            ops.train_step(ctx, P, vm, K, campos, gt, W, H, 0.2, 0.01, 0.01, grads, m, v, 1e-3, B1, B2, EPS, 1, loss)
        assert clearing_call + "(" in str(e.value)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(buffers, before))
    finally:
        clear()
        sdist.detach_native_comm(ctx)
        ctx.close()
