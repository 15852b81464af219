"""From the reference's raw parameterisation to the canonical one, on the synthetic scene.  The scene is seeded and trained
as the reference trains it -- scales and opacities rendered raw --, then Scene.activate_3dgs() turns the scales into
log-scales and the opacities into logits (scene.activations = True) and training goes on with enable_pruning=True.  From
then on the MCMC refinement, the regularisers and the renderer read the same tensors the same way: a Gaussian is "dead"
when the opacity it is RENDERED with falls to 0.005, and a relocated Gaussian gets an opacity the renderer understands.

    python examples/activated_training.py [views] [raw iterations] [activated iterations]

The refinement steps of run_3dgs_optim lie at iterations 600, 700, ... of a call, so the second phase needs more than 600
iterations to reach one.  The script prints the losses of both phases, how many Gaussians the last refinement step
relocated, and the range of the rendered opacities.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import starst3r_amd as st
from st3r_synth.synth_model import SyntheticNetwork


def main(views=4, iters_raw=300, iters_pruned=700, W=256, H=192):
    net = SyntheticNetwork(n_views=views, width=W, height=H, seed=2)
    sc = st.Scene(device="cuda:0")
    sc.add_images(net, net.images())
    sc.init_3dgs()                                                   # raw: scales 3e-3, opacities 1
    raw = sc.run_3dgs_optim(iters_raw)
    sc.activate_3dgs()                                               # logs and logits from here on; Adam's moments of the two restart
    relocated = []
    post = sc.strategy.step_post_backward

    def counting(params, optimizers, state, step, info, lr):
        post(params, optimizers, state, step, info, lr)
        if sc.strategy.is_refine_step(step):
            relocated.append(state["n_relocated"])
    sc.strategy.step_post_backward = counting
    try:
        act = sc.run_3dgs_optim(iters_pruned, enable_pruning=True)
    finally:
        del sc.strategy.step_post_backward
    torch.cuda.synchronize()
    _, _, info = sc.render_3dgs_original(W, H)
    lo, hi = float(info["opacities"].min()), float(info["opacities"].max())
    n = sc.gaussians["means"].shape[0]
    print(f"raw: loss {raw[0]:.4f} -> {raw[-1]:.4f}; activated, with pruning: {act[0]:.4f} -> {act[-1]:.4f}")
    print(f"refinement steps relocated {relocated} Gaussians; {n} Gaussians, rendered opacities in [{lo:.4f}, {hi:.4f}]")
    return dict(loss_raw=raw[-1], loss_activated=act[-1], n_relocated=sum(relocated), n_refinements=len(relocated),
                min_rendered_opacity=lo, max_rendered_opacity=hi)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    main(*a)
