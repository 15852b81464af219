"""Hand-built inputs for the condensation kernels (csrc/condense.hip): the workgroup shapes of the focal solve's counter
barrier, the nan_to_num branch, the canonical view at its block-size edges and the truncation of the anchor pixels.
test_oracle_condense_cases.py pins every case on oracle/condense_oracle.py alone; test_gpu_condense_cases.py runs them
through `ops` and asserts, through st3r_focal_plan, that each focal shape still reaches the G it was built for.

Tolerances are the existing ones of test_gpu_condense.py (float32 oracle against float32 kernel: 1e-5 on the weighted
means, 1e-4 where atan / tan / eleven dependent passes are involved, 1e-6 on one division); integer work is compared
for equality, repeated and batched launches with the same G for equal bits.
"""
import numpy as np

F = np.float32
FB_THREADS, FB_MAX_G, MAX_VIEWS = 256, 64, 1024

# (views, H, W) -> G on a whole MI355X, and what the shape is there for
FOCAL_SHAPES = [
    (1, 15, 17, 1, "255 pixels: one workgroup, last thread idle"),
    (1, 16, 16, 1, "256 pixels: one full workgroup"),
    (1, 1, 257, 2, "second workgroup owns one pixel"),
    (3, 40, 48, 8, "last workgroup half full"),
    (17, 48, 64, 12, "G not a power of two"),
    (300, 24, 32, 3, "900 workgroups"),
    (1024, 8, 8, 1, "the view limit"),
]


def plan_G(n_views, H, W, resident=None):
    """The arithmetic of st3r_focal_plan; `resident` = workgroups the device holds at once / 2 (None: unbounded)."""
    G = min(FB_MAX_G, max(1, 1024 // n_views))
    G = min(G, max(1, -(-(H * W) // FB_THREADS)))
    if resident is not None and resident < G * n_views:
        G = max(1, resident // n_views)
    return G


def pixels_of_workgroup(H, W, G, wg):
    """How many pixels workgroup `wg` of a view visits per pass (stride G * 256)."""
    p = np.arange(H * W)
    return int(((p // FB_THREADS) % G == wg).sum())


def focal_views(n_views, H, W, seed=0):
    """Exact pinhole pointmaps with a smooth depth, every view with its own focal (0.8 .. 2.5 x the 60-degree focal:
    inside the clip range 0.5 .. 3.5) and principal point (up to a pixel off the one the call passes); 2 % of the pixels
    (at least one) are pushed sideways so that the Weiszfeld weights matter.  Returns canon [n,H,W,3], pp, true focals."""
    rng = np.random.default_rng(1000 * n_views + H * W + seed)
    base = max(H, W) / (2 * np.tan(np.deg2rad(30)))
    f = base * rng.uniform(0.8, 2.5, n_views)
    cx = W / 2 + rng.uniform(-1, 1, n_views); cy = H / 2 + rng.uniform(-1, 1, n_views)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    v = np.arange(n_views)[:, None, None]
    z = 2.0 + 0.3 * np.sin(xs / 5 + v) * np.cos(ys / 4 + 0.1 * v)
    X = (xs - cx[:, None, None]) / f[:, None, None] * z
    Y = (ys - cy[:, None, None]) / f[:, None, None] * z
    canon = np.stack([X, Y, z], -1)
    n_bad = max(1, (H * W) // 50)
    for k in range(n_views):
        bad = rng.choice(H * W, n_bad, replace=False)
        canon[k].reshape(-1, 3)[bad, :2] *= rng.uniform(1.3, 2.0, (n_bad, 1))
    return np.ascontiguousarray(canon, F), (W / 2, H / 2), f


def nan_case():
    """16 x 16, z == 0 at 10 pixels (5 with x != 0: x / z = inf; 5 with x == y == 0: 0 / 0 = NaN) and z < 0 at 5."""
    canon, pp, f = focal_views(1, 16, 16, seed=3)
    c = canon[0].copy().reshape(-1, 3)
    inf_px, nan_px, neg_px = np.arange(3, 100, 20)[:5], np.arange(7, 240, 50)[:5], np.arange(11, 250, 53)[:5]
    c[inf_px, 2] = 0
    c[nan_px] = 0
    c[neg_px, 2] *= -1
    return c.reshape(16, 16, 3), pp, inf_px, nan_px, neg_px


def focal_no_nan_to_num(canon, pp):
    """oracle.estimate_focal_knowing_depth with the nan_to_num line left out (what the branch is there to prevent)."""
    H, W, _ = canon.shape
    ys, xs = np.mgrid[0:H, 0:W]
    px = np.stack([xs - F(pp[0]), ys - F(pp[1])], -1).reshape(-1, 2).astype(F)
    P = canon.reshape(-1, 3).astype(F)
    with np.errstate(all="ignore"):
        xyz = P[:, :2] / P[:, 2:3]
        dpx = (xyz * px).sum(-1); dxx = (xyz * xyz).sum(-1)
        return F(np.mean(dpx, dtype=np.float64) / np.mean(dxx, dtype=np.float64))


# ------------------------------------------------------------------------------------------------- canonical view
# (n, H, W, S): S = 1 (every pixel is its own block centre), 2, 8, S = H = W (one block); H W = 255, 256, 320
CANON_SHAPES = [(1, 15, 17, 1), (2, 15, 17, 1), (12, 17, 15, 1), (1, 16, 16, 2), (2, 16, 20, 2), (12, 16, 16, 16),
                (1, 8, 8, 8), (2, 8, 40, 8), (12, 16, 20, 4), (1, 16, 16, 16)]


def canon_case(n, H, W, S, equal_conf=False):
    """n smooth pointmaps with z in [1, 3] (z > eps at every block centre: tan(atan(.)) at pi / 2 would amplify one ulp
    without bound, so such centres are kept out of the inputs) and confidences 1.5 .. 6."""
    rng = np.random.default_rng(n * 1000 + H * W + S)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    X = np.empty((n, H, W, 3))
    for k in range(n):
        z = 2.0 + 0.8 * np.sin(xs / 3 + k) * np.cos(ys / 4 - k) + 0.05 * rng.normal(size=(H, W))
        X[k] = np.stack([(xs - W / 2) / (1.2 * W) * z, (ys - H / 2) / (1.2 * W) * z, z], -1) * (1 + 0.02 * k)
    Cf = np.full((n, H, W), 3.0) if equal_conf else rng.uniform(1.5, 6.0, (n, H, W))
    return np.ascontiguousarray(X, F), np.ascontiguousarray(Cf, F)


def block_centres(H, W, S):
    cy = np.arange(S // 2, H, S); cx = np.arange(S // 2, W, S)
    return np.ix_(cy, cx)


# ------------------------------------------------------------------------------------------------- anchor offsets
ANCHOR_N = (1, 255, 256, 257)
ANCHOR_HWS = (24, 40, 8)


def anchor_case(n):
    """xy with fractions 0.0, 0.49, 0.5, 0.999 and the largest floats below W and below H, integer parts in the first and
    the last block of each axis (and in between); canon2 distinct per pixel so that a wrong pixel shows in `off`."""
    H, W, S = ANCHOR_HWS
    rng = np.random.default_rng(n)
    canon2 = (1.0 + 0.4 * rng.uniform(-1, 1, (H, W))).astype(F)
    fr = np.array([0.0, 0.49, 0.5, 0.999])
    bx = np.array([0, 1, S - 1, S, W - S, W - 2, W - 1, W // 2 + 1]); by = np.array([0, 1, S - 1, S, H - S, H - 2, H - 1, H // 2 + 1])
    i = np.arange(n)
    x = bx[i % 8] + fr[(i // 8) % 4]; y = by[(i // 3) % 8] + fr[(i // 5) % 4]
    xy = np.stack([x, y], -1).astype(F)
    below_w, below_h = np.nextafter(F(W), F(0)), np.nextafter(F(H), F(0))
    if n == 1:
        xy[0] = (below_w, below_h)
    else:
        xy[n // 2] = (below_w, 0.5); xy[n // 2 + 1] = (0.5, below_h); xy[n - 1] = (below_w, below_h)
    return canon2, np.ascontiguousarray(xy, F), S
