"""Masked-object training on the synthetic scene: the photographs show an "object" (a disc in the middle of every view) on a
white backdrop, as a segmentation leaves them.  scene.loss_masks keeps the backdrop out of the photometric loss,
scene.backgrounds puts white under the render, and scene.alpha_masks tells the Gaussians what to be where the loss does not
look: transparent outside the disc, opaque inside it, with a ring of "don't know" pixels (scene.alpha_weights) at the edge.

    python examples/masked_object_training.py [views] [iterations]

One run in small (3 views of 128 x 96, 100 iterations, as tests/test_gpu_alpha.py runs it): mean alpha outside the object
0.766 after seeding, 0.993 after training with alpha_fac = 0 (nothing holds the dropped pixels back), 0.320 with alpha_fac = 1.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import starst3r_amd as st
from st3r_synth.synth_model import SyntheticNetwork


def outside_alpha(sc, inside, W, H):
    """mean accumulated opacity of the views' renders outside the object, 5 px away from its edge"""
    _, alpha, _ = sc.render_3dgs_original(W, H)
    far = torch.as_tensor(~inside, device=alpha.device)
    return float(alpha.detach()[..., 0][:, far].mean())


def main(views=4, iters=300, W=256, H=192, alpha_fac=1.0):
    net = SyntheticNetwork(n_views=views, width=W, height=H, seed=2)
    sc = st.Scene(device="cuda:0")
    sc.add_images(net, net.images())
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.hypot(yy - H / 2, xx - W / 2)
    disc, ring = r < 0.35 * H, np.abs(r - 0.35 * H) < 5             # the object, and the pixels nobody is sure about
    # the photographs as a segmentation leaves them: white outside the object
    sc.imgs = [np.where(disc[..., None], np.asarray(img, np.float32).reshape(H, W, 3), 1.0).astype(np.float32)
               for img in sc.imgs]
    sc.loss_masks = [disc.astype(np.float32) for _ in range(views)]
    sc.backgrounds = np.ones((views, 3), np.float32)
    sc.alpha_masks = [disc for _ in range(views)]
    sc.alpha_weights = [(~ring).astype(np.float32) for _ in range(views)]
    out = {}
    for fac in (0.0, alpha_fac):
        sc.init_3dgs()                                               # both runs from the same seeding, on the new photographs
        before = outside_alpha(sc, disc | ring, W, H)
        sc.alpha_fac = fac
        losses = sc.run_3dgs_optim(iters)
        torch.cuda.synchronize()
        out[fac] = outside_alpha(sc, disc | ring, W, H)
        print(f"alpha_fac = {fac}: loss {losses[0]:.4f} -> {losses[-1]:.4f}, mean alpha outside the object "
              f"{before:.4f} -> {out[fac]:.4f}")
    return out[0.0], out[alpha_fac]


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]]
    main(*a)
