"""'Registered for these views': the one look-up (view_reg_first, csrc/common.h) behind the seven registrations of a
context -- ground-truth moments, depth prior, exposures, intrinsics gradient, loss weights, backgrounds, alpha targets --
at its edges, once per registration, and run_3dgs_optim's clean-up when a registration itself fails.

A registration applies to a call on the registered images or on a whole-view offset into them (view chunks), and then
gives the bits of a fresh registration of exactly those views; it does not apply to the same pixels at another address,
to an offset that is no whole view, to another image size or to more views than are registered, and such a call has the
bits of the call with nothing registered.  Run on the MI355X box:
    python -m pytest tests/test_gpu_view_registration.py -m gpu -q -s
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from st3r_synth import synth
from per_view_cases import _same_bits, _setup, _small_scene, _synthetic_prior

N, V, W, H = 300, 3, 40, 24   # 3 x 2 tiles with ragged edges; H even: the images can be viewed as (V, H / 2, 2 W, 3)


class _Case:
    """one registration: how to set it for the views [k, k + n) of the scene's tensors (or of other images `gt`), how to
    clear it, and a call on n views at `gt` whose result shows whether it applied"""

    def __init__(self, kind):
        from starst3r_amd import ops
        self.kind, self.ops = kind, ops
        self.ctx = ops.Context("cuda:0")
        g, w2c, Ks = synth.make_scene(N, V, W, H, seed=7, scale_lo=0.02, scale_hi=0.08)
        self.P, self.vm, self.K, self.campos, self.gt = _setup(self.ctx, g, w2c, Ks, W, H)
        gen = torch.Generator().manual_seed(11)
        if kind == "moments":   # deliberately wrong ones: the loss gradient shows whether the kernel read them
            self.render = torch.rand((V, H, W, 3), generator=gen).cuda()
            self.payload = (0.25 * torch.rand((V, H, W, 3, 2), generator=gen).cuda(),)
        elif kind == "depth_prior":
            Z, wt, _ = _synthetic_prior(self.ctx, self.P, self.vm, self.K, W, H)
            assert all(float(wt[c].sum()) > 0 for c in range(V))
            self.payload = (Z, wt)
        elif kind == "exposure":
            E = (torch.eye(3, 4) + 0.1 * torch.randn((V, 3, 4), generator=gen)).cuda()
            self.payload = (E, torch.zeros((V, 3, 4), device="cuda:0"))
        elif kind == "intrinsics_grad":
            self.payload = (torch.zeros((V, 4), device="cuda:0"),)
        elif kind == "background":
            self.payload = (torch.rand((V, 3), generator=gen).cuda(),)
        else:   # loss_weight: the weights; alpha_target: the targets and their weights -- with holes
            maps = [torch.rand((V, H, W), generator=gen) for _ in range(1 if kind == "loss_weight" else 2)]
            maps[-1][torch.rand((V, H, W), generator=gen) < 0.3] = 0.0
            assert all(float(maps[-1][c].sum()) > 0 and float(maps[-1][c, 5:-5, 5:-5].sum()) > 0 for c in range(V))
            self.payload = tuple(m.cuda() for m in maps)
        # the buffer a call writes besides grads (its rows keep -1 where the call does not write): v_exposure, v_Ks
        self.written = {"exposure": 1, "intrinsics_grad": 0}.get(kind)

    def set(self, k=0, n=V, gt=None):
        gt = self.gt[k:k + n] if gt is None else gt
        part = [t[k:k + n] for t in self.payload]
        if self.kind == "moments":
            self.ops.set_gt_moments(self.ctx, gt, part[0].reshape(*gt.shape, 2))
        elif self.kind == "depth_prior":
            self.ops.set_depth_prior(self.ctx, gt, part[0].reshape(gt.shape[:3]), part[1].reshape(gt.shape[:3]), 0.5)
        elif self.kind == "exposure":
            self.ops.set_exposure(self.ctx, gt, *part)
        elif self.kind == "intrinsics_grad":
            self.ops.set_intrinsics_grad(self.ctx, gt, part[0])
        elif self.kind == "loss_weight":
            self.ops.set_loss_weight(self.ctx, gt, part[0].reshape(gt.shape[:3]))
        elif self.kind == "background":
            self.ops.set_background(self.ctx, gt, part[0])
        else:
            self.ops.set_alpha_target(self.ctx, gt, part[0].reshape(gt.shape[:3]), part[1].reshape(gt.shape[:3]), 0.5)

    def clear(self):
        self.ops.set_gt_moments(self.ctx, None, None)
        self.ops.set_depth_prior(self.ctx, None, None, None)
        self.ops.set_exposure(self.ctx, None, None, None)
        self.ops.set_intrinsics_grad(self.ctx, None, None)
        self.ops.set_loss_weight(self.ctx, None, None)
        self.ops.set_background(self.ctx, None, None)
        self.ops.set_alpha_target(self.ctx, None, None, None)

    def call(self, gt, k=0):
        """the gradient of a call on the views [k, k + gt.shape[0]) with the images gt (any size with H * W pixels)"""
        n, h, w = gt.shape[:3]
        if self.kind == "moments":
            _, v = self.ops.loss_l1_ssim(self.ctx, self.render[k:k + n].reshape(gt.shape), gt, 0.8, 0.2)
            out = [v]
        else:
            grads, loss = torch.empty(23 * N, device="cuda:0"), torch.zeros(1, device="cuda:0")
            if self.written is not None:
                self.payload[self.written].fill_(-1.0)   # v_exposure, v_Ks: rows a call does not write keep this
            self.ops.train_fwd_bwd(self.ctx, self.P, self.vm[k:k + n], self.K[k:k + n], self.campos[k:k + n], gt, w, h, 0.2,
                                   0.01, 0.01, grads, loss)
            out = [grads] + ([self.payload[self.written].clone()] if self.written is not None else [])
        torch.cuda.synchronize()
        return out


def _same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["moments", "depth_prior", "exposure", "intrinsics_grad", "loss_weight", "background",
                                  "alpha_target"])
def test_registration_applies_to_whole_view_slices_and_to_nothing_else(kind):
    c = _Case(kind)
    try:
        # ---- applies: the registered images and the whole-view offsets gt[1:], gt[2:]
        for k in range(V):
            part = c.gt[k:]
            c.clear()
            off = c.call(part, k)
            c.set()
            got = c.call(part, k)
            c.clear()
            c.set(k, V - k)   # a fresh registration of exactly that slice's tensors
            fresh = c.call(part, k)
            assert not _same(got, off), (kind, k, "the registration did not apply")
            assert _same(got, fresh), (kind, k)
        # ---- does not apply: the bits of the call with nothing registered
        big = torch.zeros(c.gt.numel() + 1, device="cuda:0")
        big[:-1].copy_(c.gt.reshape(-1))
        base, shifted = big[:-1].view(c.gt.shape), big[1:].view(c.gt.shape)
        assert shifted.data_ptr() == base.data_ptr() + 4
        for tag, reg, arg in (("a copy at another address", dict(), c.gt.clone()),
                              ("one float into the registered buffer", dict(gt=base), shifted),
                              ("another image size", dict(), c.gt.view(V, H // 2, 2 * W, 3)),
                              ("more views than registered", dict(k=0, n=2), c.gt)):
            c.clear()
            off = c.call(arg)
            c.set(**reg)
            got = c.call(arg)
            assert _same(got, off), (kind, tag)
        c.clear()
        off = c.call(c.gt)
        c.set()
        c.clear()
        assert _same(c.call(c.gt), off), (kind, "cleared")
    finally:
        c.clear()
        c.ctx.close()


def test_a_failing_registration_is_cleaned_up_like_a_failing_loop(monkeypatch):
    """ops.gt_moments raising (an allocation failure, say) ends run_3dgs_optim before the loop: it re-raises, nothing stays
    registered, and rows 0..3 of shN hold the compact copy the call took -- here the values from before the call, which the
    failing function overwrites first"""
    from starst3r_amd import gs as gs_mod, ops
    scene, _, _ = _small_scene()
    ctx = ops.get_context("cuda:0")
    before = scene.gaussians["shN"].detach().clone()

    def boom(*a, **k):
        scene.gaussians["shN"].data[:, :4] = 7.0
        raise RuntimeError("stop")
    monkeypatch.setattr(gs_mod.ops, "gt_moments", boom)
    with pytest.raises(RuntimeError, match="stop"):
        scene.run_3dgs_optim(2, depth_fac=1.0, exposure_lr=1e-3)
    monkeypatch.undo()
    assert ctx._gtm_keep is None and ctx._dp_keep is None and ctx._ex_keep is None
    assert _same_bits(scene.gaussians["shN"].detach(), before)
    # the library holds nothing either: a plain run equals one on a scene that never had an option
    other, _, _ = _small_scene()
    assert scene.run_3dgs_optim(2) == other.run_3dgs_optim(2)
