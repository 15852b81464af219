"""View-dependent colour at spherical-harmonics degree 3, on the synthetic scene.  scene.sh_degree = 3 makes init_3dgs
start from the canonical DC-only colours, run_3dgs_optim evaluate and train 16 rows of shN -- one more band every
`interval` steps, gsplat's trainer schedule -- and the render calls evaluate them.

    python examples/sh_degree_training.py [views] [iterations] [interval]

The script trains the same start at degree 1 and at degree 3 and prints both losses and how much of the colour each run
put into the rows above the DC term.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import starst3r_amd as st
from st3r_synth.synth_model import SyntheticNetwork


def main(views=4, iters=300, interval=50, W=256, H=192):
    net = SyntheticNetwork(n_views=views, width=W, height=H, seed=2)
    out = {}
    for degree in (1, 3):
        sc = st.Scene(device="cuda:0")
        sc.add_images(net, net.images())
        sc.sh_degree, sc.sh_degree_interval = degree, interval     # settings of the scene: set before init_3dgs
        sc.init_3dgs()
        losses = sc.run_3dgs_optim(iters)
        torch.cuda.synchronize()
        sh = sc.gaussians["shN"].data
        rows = (degree + 1) ** 2
        high = float(sh[:, 1:rows].abs().mean())
        assert not bool(sh[:, rows:].any())                          # the rows above the degree stay as initialised: zero
        print(f"degree {degree}: loss {losses[0]:.4f} -> {losses[-1]:.4f}; mean |coefficient| of rows 1..{rows - 1}: {high:.4f}")
        out[degree] = dict(loss=losses[-1], high=high)
    return out


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:4]])
