"""Hand-built Gaussians and cameras that plant the edges of the projection kernels (numpy only; torch for the float64
reference; no GPU).

Used by test_oracle_project.py (CPU: every case reaches the branch it names; the C oracle against float64 on asymmetric
cameras and clamped pairs) and test_gpu_project.py (k_project_sh_fwd of gs_project.hip, k_project_sh_bwd<false|true> of
gs_project_bwd.hip).

Cameras.  Camera 0 of most cases is the PLANTED camera: R = I, t = 0, so a Gaussian's camera coordinates are its world
coordinates and the planted equalities (z == near, m2x + radius == 0, ...) are exact in binary32.  Its focal lengths are
powers of two and its principal point is integer and OFF CENTRE:

    80 x 48:  fx 64, fy 32, cx 32 (W/2 = 40), cy 16 (H/2 = 24)      75 x 41 (ragged):  fx 64, fy 32, cx 30, cy 12

so fx != fy and the four clamp limits lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg are four different numbers
(80 x 48: 0.9375, 0.6875, 1.225, 0.725).  Camera 1 is ROVER: rotated about all three axes and translated (R is no
permutation, campos != 0), with yet another focal pair.  The cases that name their own cameras (mixed_visibility, views,
tails) use rings of look-at cameras with the same kind of intrinsics.

A case is ONE call of the kernels: the variants of a family (radius_clip_eq / radius_clip_below, views_c1 .. views_c256,
...) are cases of their own, so every test parametrises over CASES alike.  Each carries `check(case, O)`, a predicate over
the oracle's outputs O = oracle_forward(case) that proves the case reaches its branch (asserted by test_oracle_project.py).

Gradient bounds are not written down here: grad_bounds() measures them, per case, from the float32 C oracle's own chain rule
against the float64 autograd reference.
"""
import math

import numpy as np

from blend_cases import FLOOR       # 5e-5: the project's existing per-pair gradient bar

GROUPS = ("means", "quats", "scales", "opacities", "sh")
DEFAULTS = dict(eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0)
REG = (0.01, 0.01)                  # opac_fac, scale_fac of every case (reg_views = the number of cameras)
U = 2.0 ** -24                      # unit roundoff of binary32


# ---------------------------------------------------------------------------------------------------------------------
# cameras
def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def viewmat(R=None, t=(0.0, 0.0, 0.0)):
    M = np.eye(4)
    if R is not None:
        M[:3, :3] = R
    M[:3, 3] = t
    return M.astype(np.float32)


def look_at(eye, target, up=(0.1, -1.0, 0.05)):
    """OpenCV camera (x right, y down, z forward) at `eye` looking at `target`"""
    eye = np.asarray(eye, np.float64); f = np.asarray(target, np.float64) - eye; f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64)); r /= np.linalg.norm(r)
    R = np.stack([r, np.cross(f, r), f])
    return viewmat(R, -R @ eye)


def intr(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def planted_K(W, H):
    return intr(64.0, 32.0, 32.0, 16.0) if (W, H) == (80, 48) else intr(64.0, 32.0, 30.0, 12.0)


ROVER = viewmat(rot(-0.11, 0.23, 0.07), (0.3, -0.2, 0.4))


def rover_K(W, H):
    return intr(48.0, 56.0, 0.5 * W - 7.0, 0.5 * H + 5.0)


def limits(K, W, H):
    """(lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg) in float64 from the float32 intrinsics"""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    tx, ty = 0.5 * W / fx, 0.5 * H / fy
    return (W - cx) / fx + 0.3 * tx, cx / fx + 0.3 * tx, (H - cy) / fy + 0.3 * ty, cy / fy + 0.3 * ty


# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, W, H, means, quats, scales, opacities, sh, viewmats, Ks, check, **kw):
        f = lambda a: np.ascontiguousarray(a, np.float32)
        self.name, self.W, self.H = name, W, H
        self.means, self.quats, self.scales, self.opacities, self.sh = map(f, (means, quats, scales, opacities, sh))
        self.viewmats, self.Ks = f(viewmats), f(Ks)
        self.N, self.Cn = self.means.shape[0], self.viewmats.shape[0]
        self.kw = dict(DEFAULTS); self.kw.update(kw)
        self.check = check
        self.tags = {}                          # named Gaussian indices for the predicates
        for K in self.Ks:                       # asymmetric unless the case says otherwise (none does)
            assert K[0, 0] != K[1, 1] and K[0, 2] != 0.5 * W and K[1, 2] != 0.5 * H

    @property
    def reg(self):
        return (float(self.Cn),) + REG

    def campos(self):
        from oracle import gs_oracle as go
        return go.camera_positions(self.viewmats)

    def cam_coords(self):
        """[Cn, N, 3] float64 camera coordinates of the float32 inputs"""
        R = self.viewmats[:, :3, :3].astype(np.float64); t = self.viewmats[:, :3, 3].astype(np.float64)
        return np.einsum("cij,nj->cni", R, self.means.astype(np.float64)) + t[:, None, :]


class Soup:
    """Gaussians of a case, added group by group"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(4200 + seed)
        self.m, self.q, self.s, self.o, self.k = [], [], [], [], []

    def add(self, mean, scale, quat=None, opacity=None, sh=None):
        rng = self.rng
        if quat is None:                        # norm in [0.5, 2]
            quat = rng.standard_normal(4); quat *= rng.uniform(0.5, 2.0) / np.linalg.norm(quat)
        self.m.append(np.asarray(mean, np.float64)); self.q.append(np.asarray(quat, np.float64))
        self.s.append(np.broadcast_to(np.asarray(scale, np.float64), (3,)).copy())
        self.o.append(rng.uniform(0.1, 0.9) if opacity is None else opacity)
        self.k.append(rng.uniform(-0.5, 0.5, (4, 3)) if sh is None else np.asarray(sh, np.float64))
        return len(self.m) - 1

    def ordinary(self, n, zs=(1.0, 2.0, 4.0), lo=0.04, hi=0.16, xr=(-0.4, 0.6), yr=(-0.4, 0.8)):
        """n well-conditioned Gaussians inside the planted camera's image: z of 1, 2 or 4 (or `zs`), scale ratio <= 4"""
        ids = []
        for _ in range(n):
            z = float(self.rng.choice(zs))
            ids.append(self.add((self.rng.uniform(*xr) * z, self.rng.uniform(*yr) * z, z),
                                z * np.exp(self.rng.uniform(math.log(lo), math.log(hi), 3))))
        return ids

    def case(self, name, W, H, viewmats, Ks, check, **kw):
        return Case(name, W, H, np.array(self.m), np.array(self.q), np.array(self.s), np.array(self.o), np.array(self.k),
                    viewmats, Ks, check, **kw)


def two_cams(W, H):
    return np.stack([viewmat(), ROVER]), np.stack([planted_K(W, H), rover_K(W, H)])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's outputs in the kernels' dense layout
def oracle_forward(case, **override):
    """dict: vis / radii / tiles [Cn * N], records [Cn * N, 12] (the kernel's splat records: x y opacity conic.a | conic.b
    conic.c r g | b depth radius-as-int-bits 0; twelve zero floats on a culled pair), reg (float64: sum sigmoid(o),
    sum exp(s), visible pairs, reference tile intersections), packed (the oracle's own packed dict)"""
    from oracle import gs_oracle as go
    kw = dict(case.kw); kw.update(override)
    N, Cn = case.N, case.Cn
    pr = go.project_packed(case.means, case.quats, case.scales, case.viewmats, case.Ks, case.W, case.H, **kw)
    pid = pr["camera_ids"].astype(np.int64) * N + pr["gaussian_ids"]
    cols = go.sh_colors(pr["camera_ids"], pr["gaussian_ids"], case.means, case.campos(), case.sh)
    tw, th = math.ceil(case.W / 16.0), math.ceil(case.H / 16.0)
    tpg, _, _ = go.isect_tiles(pr["means2d"], pr["radii"], pr["depths"], pr["camera_ids"], 16, tw, th)
    rec = np.zeros((Cn * N, 12), np.float32)
    rec[pid, 0:2] = pr["means2d"]; rec[pid, 2] = case.opacities[pr["gaussian_ids"]]; rec[pid, 3:6] = pr["conics"]
    rec[pid, 6:9] = cols; rec[pid, 9] = pr["depths"]; rec[pid, 10] = pr["radii"].view(np.float32)
    radii = np.zeros(Cn * N, np.int32); radii[pid] = pr["radii"]
    tiles = np.zeros(Cn * N, np.int32); tiles[pid] = tpg
    o64, s64 = case.opacities.astype(np.float64), case.scales.astype(np.float64)
    reg = np.array([(1.0 / (1.0 + np.exp(-o64))).sum(), np.exp(s64).sum(), float(pid.size), float(tpg.sum())])
    return dict(vis=radii > 0, radii=radii, tiles=tiles, records=rec, reg=reg, packed=pr, pid=pid)


def cotangents(case, vis, seed=5):
    """v_splats [Cn * N, 12] float32: standard normal for (means2d, opacity, conic, colour) of the visible pairs; NaN in all
    twelve floats of every culled pair -- the kernel must skip the pair before it reads its row"""
    v = np.random.default_rng(seed).standard_normal((case.Cn * case.N, 12)).astype(np.float32)
    v[~np.asarray(vis, bool)] = np.nan
    return v


def reg_grads(case):
    """closed form of the two regularisers' gradients (float64): reg_views opac_fac / N sigma'(o), reg_views scale_fac / (3N)
    exp(s)"""
    rv, of, sf = case.reg
    sg = 1.0 / (1.0 + np.exp(-case.opacities.astype(np.float64)))
    return rv * of / case.N * sg * (1.0 - sg), rv * sf / (3.0 * case.N) * np.exp(case.scales.astype(np.float64))


def ref64(case, vis, v_splats, reg=True, campos=None, cameras=False):
    """float64 torch autograd through oracle.gs_torch_ref.project / sh_color (which hold the clamp as minimum / maximum and
    the colour clamp_min), jointly into means, quats, scales, opacities and sh; visibility is given (the C oracle's or the
    kernel's radii, as in test_gpu_pose_grad.chain_ref); the culled pairs' cotangents are never touched; campos: the float32
    camera positions the kernel was given, if not the oracle's.  cameras: also into the view matrices ("viewmats" [Cn, 4, 4],
    with campos = inverse(V)[:3, 3] INSIDE the graph, whatever `campos` says) and the intrinsics ("Ks4" [Cn, 4]: fx, fy, cx,
    cy, the clamp limits' dependence on them included) -- tests/per_view_kernel_cases.py"""
    import torch
    from oracle import gs_torch_ref as tr
    N, Cn = case.N, case.Cn
    vis = np.asarray(vis, bool).reshape(Cn, N)
    vs = torch.tensor(np.asarray(v_splats, np.float64).reshape(Cn, N, 12))
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    P = [t(case.means), t(case.quats), t(case.scales), t(case.opacities), t(case.sh.reshape(N, -1, 3)[:, :4])]
    for p in P:
        p.requires_grad_()
    means, quats, scales, opac, sh = P
    vm, K = t(case.viewmats), t(case.Ks)
    if cameras:
        k4 = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).clone().requires_grad_()
        vm.requires_grad_()
        o, l = torch.zeros(Cn, dtype=torch.float64), torch.ones(Cn, dtype=torch.float64)
        K = torch.stack([k4[:, 0], o, k4[:, 2], o, k4[:, 1], k4[:, 3], o, o, l], 1).reshape(Cn, 3, 3)
        campos = torch.inverse(vm)[:, :3, 3]
        P = P + [vm, k4]
    else:
        campos = t(case.campos() if campos is None else campos)
    outs, cots = [], []
    for c in range(Cn):
        idx = torch.tensor(np.nonzero(vis[c])[0])
        if idx.numel() == 0:
            continue
        m2, _, conic = tr.project(means[idx], quats[idx], scales[idx], vm[c], K[c], case.W, case.H, case.kw["eps2d"])
        col = tr.sh_color(means[idx], campos[c], sh[idx])
        outs += [m2, opac[idx], conic, col]
        cots += [vs[c, idx, 0:2], vs[c, idx, 2], vs[c, idx, 3:6], vs[c, idx, 6:9]]
    if outs:
        G = torch.autograd.grad(outs, P, cots, allow_unused=True)
        G = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for g, p in zip(G, P)]
    else:
        G = [np.zeros(tuple(p.shape)) for p in P]
    out = dict(zip(GROUPS + ("viewmats", "Ks4"), G))
    if reg:
        go_, gs_ = reg_grads(case)
        out["opacities"] = out["opacities"] + go_; out["scales"] = out["scales"] + gs_
    return out


def oracle_bwd(case, O, v_splats, reg=True):
    """the float32 C oracle's own chain rule (gso_project_sh_bwd: float32 forward state, double sums) on the visible pairs"""
    from oracle import gs_oracle as go
    pr, pid = O["packed"], O["pid"]
    v = np.asarray(v_splats, np.float64)[pid]
    g = go.project_sh_bwd(case.N, pr["camera_ids"], pr["gaussian_ids"], case.means, case.quats, case.scales, case.sh,
                          case.viewmats, case.Ks, case.campos(), case.W, case.H, v[:, 0:2], v[:, 3:6], v[:, 6:9], v[:, 2],
                          eps2d=case.kw["eps2d"])
    if reg:
        go_, gs_ = reg_grads(case)
        g["opacities"] = g["opacities"] + go_; g["scales"] = g["scales"] + gs_
    return g


def per_gaussian(G, R):
    """per group: (error [N], scale [N]) -- max |G - R| over the Gaussian's rows of the group, and the Gaussian's own
    max |R| floored at FLOOR x the group's maximum over the case (a Gaussian visible nowhere, or with a vanishing gradient,
    is not measured against noise)"""
    out = {}
    for k in GROUPS:
        n = R[k].shape[0]
        g, r = np.asarray(G[k], np.float64).reshape(n, -1), np.asarray(R[k], np.float64).reshape(n, -1)
        own = np.abs(r).max(1)
        scale = np.maximum(own, FLOOR * max(float(own.max()), 1e-300))
        out[k] = (np.abs(g - r).max(1), scale)
    return out


def grad_bounds(o32, r64):
    """per parameter group: rel = 4 x the worst per-Gaussian relative error of the float32 C oracle's chain rule against
    float64 on this case (the factor covers the kernel's other order -- per camera in registers -- and its FMA
    contraction), floored at FLOOR.  The floor is needed because the oracle's chain rule runs in double on a float32
    forward state: on well-conditioned Gaussians its error is a few float32 roundings of the inputs, less than ANY float32
    evaluation of the chain rule can reach.  FLOOR is the project's existing bar for these gradients
    (test_backward_vs_oracle: 5e-5) -- here of each Gaussian's own gradient, not of the tensor's maximum."""
    pg = per_gaussian(o32, r64)
    out = {}
    for k in GROUPS:
        err, scale = pg[k]
        own = float((err / scale).max())
        out[k] = dict(rel=max(4.0 * own, FLOOR), own=own, scale=scale)
    return out


_refs = {}


def reference(name):
    """computed once per case and shared, never modified: O (oracle forward), v (cotangents), r64, o32, bounds"""
    if name not in _refs:
        case = get(name)
        O = oracle_forward(case)
        v = cotangents(case, O["vis"])
        r64 = ref64(case, O["vis"], v)
        o32 = oracle_bwd(case, O, v)
        _refs[name] = dict(O=O, v=v, r64=r64, o32=o32, bounds=grad_bounds(o32, r64))
    return _refs[name]


# ---------------------------------------------------------------------------------------------------------------------
# predicates' helpers
def vis_of(case, O, cam=0):
    return set(np.nonzero(O["vis"].reshape(case.Cn, case.N)[cam])[0].tolist())


def f32(x):
    return np.float32(x)


def m2_f32(K, p):
    """the kernel's own three float32 operations for means2d, from float32 camera coordinates p (planted camera: = mean)"""
    rz = f32(1.0) / f32(p[2])
    return f32(f32(K[0, 0] * f32(p[0])) * rz) + K[0, 2], f32(f32(K[1, 1] * f32(p[1])) * rz) + K[1, 2]


def probe_radius(case, g):
    """radius (and conic) of Gaussian g in the planted camera with the screen test out of the way: the same camera with a
    principal point moved by (W, H) inside an image of (4W, 4H) -- an UNCLAMPED pair's cov2d does not depend on either"""
    from oracle import gs_oracle as go
    K = case.Ks[0].copy(); K[0, 2] += case.W; K[1, 2] += case.H
    kw = dict(case.kw); kw["radius_clip"] = 0.0
    pr = go.project_packed(case.means[g:g + 1], case.quats[g:g + 1], case.scales[g:g + 1], case.viewmats[0:1], K[None],
                           4 * case.W, 4 * case.H, **kw)
    assert pr["radii"].shape[0] == 1
    return int(pr["radii"][0])


def clamp_sides(case, O):
    """per visible pair: which limit it lies beyond (xp, xn, yp, yn: bool [Cn * N]) and the smallest relative distance of
    any visible pair's x/z, y/z to any of its camera's four limits"""
    pc = case.cam_coords()
    xr, yr = pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2]
    L = np.array([limits(K, case.W, case.H) for K in case.Ks])[:, None, :]
    vis = O["vis"].reshape(case.Cn, case.N)
    sides = dict(xp=(xr > L[..., 0]) & vis, xn=(xr < -L[..., 1]) & vis, yp=(yr > L[..., 2]) & vis, yn=(yr < -L[..., 3]) & vis)
    d = np.stack([np.abs(xr / L[..., 0] - 1), np.abs(xr / L[..., 1] + 1), np.abs(yr / L[..., 2] - 1), np.abs(yr / L[..., 3] + 1)])
    near = float(d[:, vis].min()) if vis.any() else 1.0
    return sides, near


def generic_check(case, O):
    assert O["vis"].any()


# ---------------------------------------------------------------------------------------------------------------------
# the cases
def near_far():
    W, H = 80, 48
    s = Soup(1)
    near, far = f32(0.5), f32(4.0)
    zs = [near, np.nextafter(near, f32(0)), far, np.nextafter(far, f32(np.inf))]
    ids = [s.add((0.125 * float(z), 0.0625 * float(z), float(z)), np.array([0.08, 0.05, 0.03]) * float(z)) for z in zs]
    s.ordinary(8)
    vm, Ks = two_cams(W, H)

    def check(case, O):
        assert [float(case.means[i, 2]) for i in ids] == [0.5, float(zs[1]), 4.0, float(zs[3])]
        assert zs[1] < near and zs[3] > far
        v = vis_of(case, O)
        assert ids[0] in v and ids[2] in v and ids[1] not in v and ids[3] not in v       # the cull is z < near, z > far
        allv = vis_of(case, oracle_forward(case, near=0.01, far=1e10))
        assert set(ids) <= allv                                                       # nothing else culls the four
        dead = [c * case.N + i for c in (0,) for i in (ids[1], ids[3])]
        assert not O["records"][dead].any() and not O["tiles"][dead].any()
    return s.case("near_far", W, H, vm, Ks, check, near=0.5, far=4.0)


def screen_edges():
    """per side: a pair with exactly m2x + radius == 0 (m2x - radius == W, m2y + radius == 0, m2y - radius == H), culled,
    and its neighbour towards the image, kept: the mean moved by the fewest floats that move m2x / m2y at all (one or two;
    at most 8 floats of m2x).  All eight are unclamped (their x/z, y/z lie inside
    the limits), so the radius the probe camera reports is the radius of the culled pair."""
    W, H = 80, 48
    K = planted_K(W, H)
    s = Soup(2)
    z, sc = 2.0, np.array([0.0625, 0.04, 0.025])      # sigma <= 64 * 0.0625 / 2 = 2 px: radius 7 or so
    pairs = {}
    for side in ("left", "right", "top", "bottom"):
        r = 7
        qs = s.rng.standard_normal(4)
        for _ in range(4):                    # the radius depends (weakly) on the position: fixed point
            if side == "left":
                mean = (-(r + 32.0) * z / 64.0, 0.25 * z, z)
            elif side == "right":
                mean = ((W + r - 32.0) * z / 64.0, 0.25 * z, z)
            elif side == "top":
                mean = (0.25 * z, -(r + 16.0) * z / 32.0, z)
            else:
                mean = (0.25 * z, (H + r - 16.0) * z / 32.0, z)
            i = s.add(mean, sc, quat=qs)
            tmp = s.case("tmp", W, H, *two_cams(W, H), generic_check)
            r_new = probe_radius(tmp, i)
            for lst in (s.m, s.q, s.s, s.o, s.k):
                lst.pop()
            if r_new == r:
                break
            r = r_new
        i = s.add(mean, sc, quat=qs)
        m = np.asarray(mean, np.float32)
        ax = 0 if side in ("left", "right") else 1
        for _ in range(4):                    # (one float of the mean can be half a float of m2x: step until m2x moves)
            m[ax] = np.nextafter(m[ax], f32(np.inf) if side in ("left", "top") else f32(-np.inf))
            if m2_f32(K, m)[ax] != m2_f32(K, np.asarray(mean, np.float32))[ax]:
                break
        j = s.add(m.astype(np.float64), sc, quat=qs)
        pairs[side] = (i, j)
    s.ordinary(8)
    vm, Ks = two_cams(W, H)

    def check(case, O):
        v = vis_of(case, O)
        sides, _ = clamp_sides(case, O)
        for side, (i, j) in pairs.items():
            r = probe_radius(case, i)
            assert r == probe_radius(case, j) == int(O["radii"][j])
            x, y = m2_f32(case.Ks[0], case.means[i])
            xj, yj = m2_f32(case.Ks[0], case.means[j])
            if side == "left":
                assert f32(x + f32(r)) == 0.0 and f32(xj + f32(r)) > 0.0
            elif side == "right":
                assert f32(x - f32(r)) == f32(W) and f32(xj - f32(r)) < f32(W)
            elif side == "top":
                assert f32(y + f32(r)) == 0.0 and f32(yj + f32(r)) > 0.0
            else:
                assert f32(y - f32(r)) == f32(H) and f32(yj - f32(r)) < f32(H)
            assert i not in v and j in v, side
            assert (O["records"][j, 0], O["records"][j, 1]) == (xj, yj)
            # unclamped: the limits are not what culls or shapes them
            pc = case.cam_coords()[0, [i, j]]
            L = limits(case.Ks[0], W, H)
            assert (pc[:, 0] / pc[:, 2] < L[0]).all() and (pc[:, 0] / pc[:, 2] > -L[1]).all()
            assert (pc[:, 1] / pc[:, 2] < L[2]).all() and (pc[:, 1] / pc[:, 2] > -L[3]).all()
    return s.case("screen_edges", W, H, vm, Ks, check)


def _radius_clip(which):
    W, H = 75, 41
    s = Soup(3)
    g = s.add((0.25, 0.125, 2.0), (0.3, 0.2, 0.25))
    s.ordinary(8)
    vm, Ks = two_cams(W, H)
    probe = s.case("tmp", W, H, vm, Ks, generic_check)
    r = int(oracle_forward(probe)["radii"][g])
    assert r > 3
    clip = float(r) if which == "eq" else float(r - 1)

    def check(case, O):
        assert case.kw["radius_clip"] == clip
        free = oracle_forward(case, radius_clip=0.0)
        assert int(free["radii"][g]) == r
        assert (g in vis_of(case, O)) == (which == "below")          # radius <= radius_clip culls
        # the clip culls others too; every pair it leaves has a larger radius
        assert (O["radii"][O["vis"]] > clip).all() and (free["radii"][free["vis"] & ~O["vis"]] <= clip).all()
    return s.case("radius_clip_" + which, W, H, vm, Ks, check, radius_clip=clip)


def _det_zero(eps2d):
    """planted camera = identity view matrix; g0: axis-aligned, scales (0, s, s), on the optical axis: c00 == 0 and c01 == 0,
    det == 0 exactly without eps2d; g1: all scales 0"""
    W, H = 80, 48
    s = Soup(4)
    g0 = s.add((0.0, 0.0, 2.0), (0.0, 0.25, 0.25), quat=(2.0, 0.0, 0.0, 0.0))
    g1 = s.add((0.25, 0.125, 2.0), (0.0, 0.0, 0.0))
    s.ordinary(10, lo=0.06, hi=0.2)
    vm, Ks = two_cams(W, H)

    def check(case, O):
        v = vis_of(case, O)
        if eps2d == 0.0:
            assert g0 not in v and g1 not in v
            assert not O["records"][[g0, g1]].any()
            assert len(v) >= 8
        else:
            assert g0 in v and g1 in v
            e = np.float32(0.3)
            inv = np.float32(1.0) / np.float32(e * e)                # conic of cov2d = eps2d I: (1 / 0.3, 0, 1 / 0.3)
            for c in range(case.Cn):
                if O["vis"][c * case.N + g1]:
                    assert O["records"][c * case.N + g1, 3:6].tolist() == [e * inv, 0.0, e * inv]
            np.testing.assert_allclose(O["records"][g1, [3, 5]], 1.0 / 0.3, rtol=4 * U)
            a, b, cc = (float(x) for x in O["records"][g0, 3:6])
            assert b == 0.0 and abs(a - 1.0 / 0.3) <= 8 * U / 0.3 and 0 < cc < a      # c00 = 0 + eps2d: conic.a = 1 / eps2d
    return s.case("det_zero_eps%s" % ("0" if eps2d == 0.0 else "03"), W, H, vm, Ks, check, eps2d=eps2d)


def _clamp(side):
    W, H = (80, 48) if side in ("xp", "yp") else (75, 41)
    K = planted_K(W, H)
    Lxp, Lxn, Lyp, Lyn = limits(K, W, H)
    s = Soup(10 + ("xp", "xn", "yp", "yn").index(side))
    rng = s.rng
    big = []
    for i in range(12):
        z = float(rng.choice([1.0, 2.0, 4.0]))
        f = 1.02 + 0.1 * i / 11.0                                     # x/z or y/z = limit * f: 2 % .. 12 % beyond it
        x, y = rng.uniform(-0.2, 0.4), rng.uniform(-0.1, 0.5)
        if side == "xp": x = Lxp * f
        if side == "xn": x = -Lxn * f
        if side == "yp": y = Lyp * f
        if side == "yn": y = -Lyn * f
        # sigma >= 64 * 0.13 = 8.3 px: a radius of 25 px or more reaches the image from at most 18 px outside it, and the
        # conic stays large enough (1 / 70 .. 1 / 200) for the clamped Jacobian's terms to weigh in the mean's gradient --
        # with Gaussians of 30 px the `else` terms of x_in / y_in were below the bound
        big.append(s.add((x * z, y * z, z), z * rng.uniform(0.13, 0.22, 3)))
    s.ordinary(12)
    vm, Ks = two_cams(W, H)

    def check(case, O):
        sides, near = clamp_sides(case, O)
        vis0 = O["vis"][:case.N]
        assert int(sides[side][0].sum()) >= 8, (side, int(sides[side][0].sum()))     # in the planted camera alone
        assert near > 1e-3, near
        unclamped = vis0 & ~np.any([sides[k][0] for k in sides], axis=0)
        assert int(unclamped.sum()) >= 8
        L = limits(case.Ks[0], W, H)
        assert len({round(v, 6) for v in L}) == 4                    # four different limits
    return s.case("clamp_" + side, W, H, vm, Ks, check)


def quat_norm():
    W, H = 75, 41
    s = Soup(20)
    ids = s.ordinary(16)
    norms = np.logspace(-3, 3, 15)
    for i, n in zip(ids[:15], norms):
        s.q[i] = s.q[i] / np.linalg.norm(s.q[i]) * n
    s.q[ids[15]] = np.array([0.5, -0.5, 0.5, 0.5])                   # already unit, exactly
    vm, Ks = two_cams(W, H)

    def check(case, O):
        n = np.linalg.norm(case.quats.astype(np.float64), axis=1)
        assert n.min() < 1.1e-3 and n.max() > 0.9e3
        q = case.quats[ids[15]]
        assert float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) == 1.0
        assert len(vis_of(case, O)) >= 12
    return s.case("quat_norm", W, H, vm, Ks, check)


SH_C0, SH_C1 = 0.2820947917738781, 0.48860251190292


def colour_pre(case):
    """[Cn, N, 3] float64: the colour before the clamp"""
    d = case.means.astype(np.float64)[None] - case.campos().astype(np.float64)[:, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    k = case.sh.reshape(case.N, -1, 3)[:, :4].astype(np.float64)
    x, y, z = d[..., 0:1], d[..., 1:2], d[..., 2:3]
    return SH_C0 * k[None, :, 0] + SH_C1 * (-y * k[None, :, 1] + z * k[None, :, 2] - x * k[None, :, 3]) + 0.5


def colour_clamp():
    """Gaussian i: i % 4 channels whose colour is below 0 in every camera (DC coefficient -4: pre <= -0.37), the others
    above (DC +1: pre >= 0.52); the last 8: DC -0.5 / SH_C0 and direction coefficients of +-1.5, so that the sign of a
    channel differs between the planted camera and a third one that looks from the side"""
    W, H = 75, 41
    s = Soup(21)
    ids = s.ordinary(24)
    for n, i in enumerate(ids):
        k = s.rng.uniform(-0.3, 0.3, (4, 3))
        if n < 16:
            k[0] = 1.0
            k[0, :n % 4] = -4.0
        else:
            k[0] = -0.5 / SH_C0
            k[1:] = s.rng.choice([-1.5, 1.5], (3, 3))
        s.k[i] = k
    vm, Ks = two_cams(W, H)
    vm = np.concatenate([vm, look_at((3.0, -0.3, 2.0), (0.0, 0.2, 2.2))[None]])      # from the side: other directions
    Ks = np.concatenate([Ks, intr(40.0, 64.0, 30.0, 26.0)[None]])

    def check(case, O):
        pre = colour_pre(case).reshape(-1, 3)[O["vis"]]
        assert np.abs(pre).min() >= 1e-3, np.abs(pre).min()
        col = O["records"][O["vis"], 6:9]
        assert np.array_equal(col == 0, pre < 0)
        cnt = np.bincount((pre < 0).sum(1), minlength=4)
        assert (cnt >= 4).all(), cnt                                 # pairs with 0, 1, 2 and all 3 channels clamped
        p = colour_pre(case)
        v = O["vis"].reshape(case.Cn, case.N)
        assert int((((p[0] < 0) != (p[2] < 0)).any(-1) & v[0] & v[2]).sum()) >= 2      # clamped in one camera, not in the other
    return s.case("colour_clamp", W, H, vm, Ks, check)


def ring(Cn, W, H, radius=3.0, seed=0):
    """Cn look-at cameras on a wobbling ring around the origin, intrinsics varied per camera (never symmetric)"""
    rng = np.random.default_rng(77 + seed)
    vms, Ks = [], []
    for c in range(Cn):
        az = 2 * math.pi * c / Cn + 0.1
        eye = (radius * math.cos(az), 0.5 * math.sin(3 * az) + 0.2, radius * math.sin(az))
        vms.append(look_at(eye, rng.uniform(-0.2, 0.2, 3)))
        fx = (0.75, 1.0, 1.25)[c % 3] * W
        Ks.append(intr(fx, fx * (0.625, 0.8)[c % 2], 0.5 * W + (-7.0, 5.0, 9.0)[c % 3], 0.5 * H + (4.0, -6.0)[c % 2]))
    return np.stack(vms), np.stack(Ks)


def mixed_visibility():
    """three cameras looking along +z, +x (turned and tilted) and -z: every Gaussian of groups A, B, C is in front of one or
    two of them and behind or beside the rest; group D is visible nowhere (high above all three)"""
    W, H = 80, 48
    s = Soup(22)
    rng = s.rng
    for _ in range(10):
        s.add((rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(1.5, 3.0)), rng.uniform(0.08, 0.2, 3))     # A
        s.add((rng.uniform(1.5, 3.0), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5)), rng.uniform(0.08, 0.2, 3))     # B
        s.add((rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(-3.0, -1.5)), rng.uniform(0.08, 0.2, 3))   # C
    D = [s.add((rng.uniform(-1, 1), -40.0, rng.uniform(-1, 1)), rng.uniform(0.08, 0.2, 3)) for _ in range(6)]
    vms = np.stack([viewmat(), look_at((-0.4, 0.1, 0.2), (2.0, 0.0, 0.3)), look_at((0.2, -0.1, 0.5), (0.0, 0.1, -2.0))])
    Ks = np.stack([planted_K(W, H), rover_K(W, H), intr(40.0, 64.0, 46.0, 20.0)])

    def check(case, O):
        vis = O["vis"].reshape(case.Cn, case.N)
        nowhere = ~vis.any(0)
        assert set(np.nonzero(nowhere)[0].tolist()) == set(D)
        rest = ~nowhere
        assert (vis.any(0) & ~vis.all(0))[rest].all()                # culled in a camera, visible in another
        for c in range(case.Cn - 1):                                 # culled in one camera and visible in the NEXT
            assert int((~vis[c] & vis[c + 1]).sum()) >= 4 and int((vis[c] & ~vis[c + 1]).sum()) >= 4
        assert vis[:, :].sum(1).min() >= 8
    return s.case("mixed_visibility", W, H, vms, Ks, check)


def _cloud(s, n, extent=0.6, lo=0.04, hi=0.16, stray=7):
    """n Gaussians around the origin; every `stray`-th one 2 away from it in a random direction: outside some cameras'
    images"""
    for i in range(n):
        m = s.rng.uniform(-extent, extent, 3)
        if i % stray == stray - 1:
            m = s.rng.standard_normal(3); m *= 2.0 / np.linalg.norm(m)
        s.add(m, np.exp(s.rng.uniform(math.log(lo), math.log(hi), 3)))


def _views(Cn):
    W, H = (32, 32) if Cn == 256 else (80, 48)
    s = Soup(30)
    _cloud(s, 65)
    vms, Ks = ring(Cn, W, H, seed=Cn)

    def check(case, O):
        assert case.Cn == Cn and case.N == 65
        vis = O["vis"].reshape(Cn, 65)
        assert vis.sum(1).min() >= 8                                 # every camera sees something
        assert not vis.all()                                         # and some pairs are culled
    return s.case("views_c%d" % Cn, W, H, vms, Ks, check)


def _tails(N):
    W, H = 75, 41
    s = Soup(40 + N)
    _cloud(s, N, extent=0.9)
    vms, Ks = ring(2, W, H, seed=1)

    def check(case, O):
        assert case.N == N and case.Cn == 2
        vis = O["vis"].reshape(2, N)
        assert vis[:, N - 1].any() and vis[:, 0].any()               # the first and the last Gaussian are not idle
        assert N < 8 or not vis.all()
    return s.case("tails_n%d" % N, W, H, vms, Ks, check)


def _sh_stride(rows):
    W, H = 80, 48
    s = Soup(50)
    s.ordinary(40)
    vm, Ks = two_cams(W, H)
    c = s.case("sh_stride_%d" % (3 * rows), W, H, vm, Ks, None)
    if rows > 4:
        full = np.full((c.N, rows, 3), np.nan, np.float32); full[:, :4] = c.sh
        c.sh = full

    def check(case, O):
        assert case.sh.shape == (case.N, rows, 3) and int(np.prod(case.sh.shape[1:])) == 3 * rows
        assert np.isnan(case.sh[:, 4:]).all() and np.isfinite(case.sh[:, :4]).all()
        assert np.isfinite(O["records"]).all() and O["vis"].sum() >= 40
    c.check = check
    return c


def _regulariser(N):
    """raw opacities in [-8, 8] (the reference renders them raw) and log-scales in [-6, 1]: the values the two regularisers
    see; the projection takes the same numbers as they are.  N = 257: two blocks feed k_reg_reduce, N = 1000: four."""
    W, H = 80, 48
    s = Soup(60 + N)
    rng = s.rng
    for _ in range(N):
        z = rng.uniform(2.0, 6.0)
        s.add((rng.uniform(-0.8, 1.0) * z, rng.uniform(-0.8, 1.2) * z, z), rng.uniform(-6.0, 1.0, 3),
              opacity=rng.uniform(-8.0, 8.0))
    vm, Ks = two_cams(W, H)

    def check(case, O):
        assert case.N == N and math.ceil(N / 256) >= 2
        assert case.opacities.min() < -7 and case.opacities.max() > 7
        assert case.scales.min() < -5.5 and case.scales.max() > 0.9
        assert 0 < O["reg"][2] < case.Cn * N and O["reg"][3] > O["reg"][2]
    return s.case("regulariser_n%d" % N, W, H, vm, Ks, check)


CASES = {"near_far": near_far, "screen_edges": screen_edges,
         "radius_clip_eq": lambda: _radius_clip("eq"), "radius_clip_below": lambda: _radius_clip("below"),
         "det_zero_eps0": lambda: _det_zero(0.0), "det_zero_eps03": lambda: _det_zero(0.3),
         "clamp_xp": lambda: _clamp("xp"), "clamp_xn": lambda: _clamp("xn"), "clamp_yp": lambda: _clamp("yp"),
         "clamp_yn": lambda: _clamp("yn"), "quat_norm": quat_norm, "colour_clamp": colour_clamp,
         "mixed_visibility": mixed_visibility}
for _c in (1, 8, 9, 64, 256):
    CASES["views_c%d" % _c] = (lambda c: lambda: _views(c))(_c)
for _n in (1, 63, 64, 65, 255, 256, 257):
    CASES["tails_n%d" % _n] = (lambda n: lambda: _tails(n))(_n)
CASES["sh_stride_12"] = lambda: _sh_stride(4)
CASES["sh_stride_72"] = lambda: _sh_stride(24)
for _n in (257, 1000):
    CASES["regulariser_n%d" % _n] = (lambda n: lambda: _regulariser(n))(_n)

_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# scenes of the fused path (st3r_gs_train_fwd_bwd takes no projection options: defaults throughout)
FUSED_N = (1, 63, 64, 65, 255, 257)


def fused_shape(N):
    """N Gaussians, two ring cameras, 48 x 32: several tiles per pair, nothing saturates"""
    W, H = 48, 32
    s = Soup(70 + N)
    if N == 1:
        s.add((0.05, -0.02, 0.1), (0.25, 0.15, 0.2), opacity=0.6)
    else:
        _cloud(s, N, extent=0.7, lo=0.05, hi=0.2)
    vms, Ks = ring(2, W, H, radius=2.5, seed=2)
    return s.case("fused_n%d" % N, W, H, vms, Ks, generic_check)


GATHER_BIG = (0, 7, 15, 23, 31, 40, 50, 63)       # lanes 0 and 63 own slots: lane 63 closes a non-empty range


def gather_scene(which):
    """One wave (N = 64), one camera, the slot count of the wave planted on both sides of 64 * GATHER_WIDE_ABOVE = 384:

      gather_384     128 x 96 (48 tiles): 8 Gaussians of opacity 0.1 (nothing saturates: T >= 0.43) whose alpha passes 1/255
                     at a pixel centre of EVERY tile (sigma >= 44 px in x, 33 px in y, centred within 4 px of the image
                     centre: Mahalanobis^2 <= 2.5 at the far corner tiles' nearest pixel against ln(25.5) * 2 = 6.5), the
                     other 56 behind the camera: 384 slots, the narrow form;
      gather_385     the same with Gaussian 32 brought to the front as a one-tile Gaussian: 385 slots, the wide form;
      gather_uneven  176 x 96 (66 tiles): 6 such Gaussians, each ONE pair of 66 slots between empty pairs -- its range
                     spans two or three 64-slot chunks of the wide form -- and three one-tile Gaussians: 399 slots."""
    W, H = (176, 96) if which == "uneven" else (128, 96)
    s = Soup(80)
    rng = s.rng
    K = intr(128.0, 64.0, 0.5 * W - 6.0, 0.5 * H + 4.0)
    big = GATHER_BIG if which != "uneven" else (3, 13, 24, 35, 46, 60)
    small = {"384": (), "385": (32,), "uneven": (8, 30, 52)}[which]
    z = 2.0
    for i in range(64):
        if i in big:
            px, py = 0.5 * W + rng.uniform(-4, 4), 0.5 * H + rng.uniform(-4, 4)
            mean = ((px - K[0, 2]) * z / 128.0, (py - K[1, 2]) * z / 64.0, z)
            s.add(mean, (rng.uniform(0.7, 0.9) * (1.6 if which == "uneven" else 1.0), rng.uniform(1.1, 1.4), rng.uniform(0.8, 1.2)),
                  quat=(1.0, 0.02 * rng.standard_normal(), 0.02 * rng.standard_normal(), 0.02 * rng.standard_normal()),
                  opacity=0.1)
        else:
            s.add((rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(1.0, 3.0)), rng.uniform(0.1, 0.3, 3))
    for n, i in enumerate(small):                    # one tile: centred on a tile centre, 3 sigma = 5 px
        px, py = 16.0 * (2 + 2 * n) + 8.0, 16.0 * (1 + n) + 8.0
        s.m[i] = np.array([(px - K[0, 2]) * z / 128.0, (py - K[1, 2]) * z / 64.0, z])
        s.s[i] = np.array([0.018, 0.036, 0.02]); s.q[i] = np.array([1.0, 0.0, 0.0, 0.0]); s.o[i] = 0.5
    c = s.case("gather_" + which, W, H, viewmat()[None], K[None], generic_check)
    c.tags = dict(big=big, small=small, tiles=math.ceil(W / 16) * math.ceil(H / 16))
    return c


def stage_bounds(stage, r64, fused_floor=2e-5):
    """per group: max(4 x max |stage - float64| over the group, 2e-5 x the group's max |stage|) -- the fused kernel sums the
    same slots in the same order, so it may differ from the stage path by no more than the stage path's own float32 error;
    2e-5 is the project's existing figure for fused against stage grouping (test_fused_train_gradients_equal_stage_path)"""
    out = {}
    for k in GROUPS:
        a, r = np.asarray(stage[k], np.float64), np.asarray(r64[k], np.float64)
        own = float(np.abs(a - r).max())
        out[k] = dict(abs=max(4.0 * own, fused_floor * float(np.abs(a).max())), own=own, scale=float(np.abs(a).max()))
    return out
