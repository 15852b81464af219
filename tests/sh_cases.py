"""Spherical harmonics of degree 0..3 (st3r_ctx_set_sh_degree): the basis, its float64 autograd reference, a float32
restatement of the kernels' chain rule, and the planted cases (numpy and float64 torch; no GPU).

Used by test_host_sh_degree.py (CPU: the cases reach the edges they name, the restatement is the autograd reference's
chain rule) and test_gpu_sh_degree.py (k_project_sh_fwd<DEG>, k_project_sh_bwd<GATHER, DEG>, k_viewmat_bwd_part<DEG>).
oracle/gs_oracle.py asserts degree 1 and is not involved: which pairs are visible is its project_packed's answer (the
geometry does not depend on the degree), the colours and their gradients are this file's.

The basis, u = normalise(mean - campos) = (x, y, z):
    row 0       C0                                  rows 1..3   C1 (-y, z, -x)
    rows 4..8   C2[i] (xy, yz, 2zz - xx - yy, xz, xx - yy)
    rows 9..15  C3[i] (y(3xx - yy), xyz, y(4zz - xx - yy), z(2zz - 3xx - 3yy), x(4zz - xx - yy), z(xx - yy), x(xx - 3yy))
colour = clamp_min(sum over the K = (deg + 1)^2 rows + 0.5, 0).

Cameras are project_cases.py's: one camera = the planted 80 x 48 camera (R = I at the origin), two = planted + ROVER,
nine = the look-at ring.  Planted Gaussians, in front of everything else a case holds (those a case has room for):
    axis      straight ahead of the planted camera: u = (0, 0, 1) exactly, every basis function with a factor x or y is 0;
              nine cameras: along -x from ring camera 0's centre and along +y from camera Y_CAM's (a look-at camera that
              looks down the y axis, in the ring's place 5), the other two components 0.0 exactly
    plane     x = 0 or y = 0 in the planted camera's frame: the basis functions with that factor are 0
    close     1e-3 in front of the LAST camera's centre, 1e-6 small (near = 1e-4 in every case, so that the pair is
              visible): 1 / |d| = 1000 in the direction's chain rule
    culled    the first two Gaussians of the crowd that are outside one camera's image and inside another's (two and
              nine cameras; the crowd is drawn wider than the image)
Every Gaussian's DC coefficients are drawn so that its pairs have 0, 1, 2 or 3 channels clamped (g % 4, the rest left to
the view), and every channel of every visible pair has |pre-clamp| >= 1e-3 in float64: coefficients are redrawn until
that holds, so the float32 kernel takes the same branch and no pair is left out of a comparison.
"""
import math

import numpy as np

import project_cases as pc
from project_cases import FLOOR

C0, C1 = 0.2820947917738781, 0.48860251190292
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)
W, H = 80, 48
NS, CS, DEGREES = (1, 255, 256, 257, 1000), (1, 2, 9), (0, 1, 2, 3)
NEAR = 1e-4
MARGIN = 1e-3
Y_CAM = 5                           # of the nine cameras: the one that looks along +y
GROUPS = ("sh", "means", "viewmats")


def rows(deg):
    return (deg + 1) ** 2


def basis(x, y, z, deg):
    """the rows(deg) basis functions, constants included, at the unit direction (x, y, z): numpy arrays or torch tensors"""
    b = [C0 + 0.0 * x]
    if deg >= 1:
        b += [-C1 * y, C1 * z, -C1 * x]
    xx, yy, zz = x * x, y * y, z * z
    if deg >= 2:
        b += [C2[0] * (x * y), C2[1] * (y * z), C2[2] * (2.0 * zz - xx - yy), C2[3] * (x * z), C2[4] * (xx - yy)]
    if deg >= 3:
        b += [C3[0] * (y * (3.0 * xx - yy)), C3[1] * (x * y * z), C3[2] * (y * (4.0 * zz - xx - yy)),
              C3[3] * (z * (2.0 * zz - 3.0 * xx - 3.0 * yy)), C3[4] * (x * (4.0 * zz - xx - yy)), C3[5] * (z * (xx - yy)),
              C3[6] * (x * (xx - 3.0 * yy))]
    return b


def basis_grad(x, y, z, deg):
    """per row (d/dx, d/dy, d/dz) of basis(), as polynomials in three free variables (numpy)"""
    o = 0.0 * x
    g = [(o, o, o)]
    if deg >= 1:
        g += [(o, o - C1, o), (o, o, o + C1), (o - C1, o, o)]
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    if deg >= 2:
        g += [(C2[0] * y, C2[0] * x, o), (o, C2[1] * z, C2[1] * y), (C2[2] * -2.0 * x, C2[2] * -2.0 * y, C2[2] * 4.0 * z),
              (C2[3] * z, o, C2[3] * x), (C2[4] * 2.0 * x, C2[4] * -2.0 * y, o)]
    if deg >= 3:
        g += [(C3[0] * 6.0 * xy, C3[0] * (3.0 * xx - 3.0 * yy), o), (C3[1] * yz, C3[1] * xz, C3[1] * xy),
              (C3[2] * -2.0 * xy, C3[2] * (4.0 * zz - xx - 3.0 * yy), C3[2] * 8.0 * yz),
              (C3[3] * -6.0 * xz, C3[3] * -6.0 * yz, C3[3] * (6.0 * zz - 3.0 * xx - 3.0 * yy)),
              (C3[4] * (4.0 * zz - 3.0 * xx - yy), C3[4] * -2.0 * xy, C3[4] * 8.0 * xz),
              (C3[5] * 2.0 * xz, C3[5] * -2.0 * yz, C3[5] * (xx - yy)), (C3[6] * (3.0 * xx - 3.0 * yy), C3[6] * -6.0 * xy, o)]
    return g


def directions(means, campos, dtype=np.float64):
    """(u [Cn, N, 3], 1 / |d| [Cn, N]) in dtype"""
    d = means.astype(dtype)[None] - campos.astype(dtype)[:, None]
    inrm = (dtype(1.0) / np.sqrt((d * d).sum(-1))).astype(dtype)
    return d * inrm[..., None], inrm


def pre_clamp(means, campos, sh, deg, dtype=np.float64):
    """[Cn, N, 3]: sum over the rows in use + 0.5"""
    u, _ = directions(means, campos, dtype)
    b = np.stack(basis(u[..., 0], u[..., 1], u[..., 2], deg)).astype(dtype)            # [K, Cn, N]
    return (np.einsum("kcn,nkj->cnj", b, sh[:, :rows(deg)].astype(dtype)) + dtype(0.5)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# cases
def cameras(Cn):
    if Cn == 1:
        return pc.viewmat()[None], pc.planted_K(W, H)[None]
    if Cn == 2:
        return pc.two_cams(W, H)
    vms, Ks = pc.ring(Cn, W, H, seed=Cn)
    # ring camera Y_CAM gives its place to a look-at camera above the scene looking straight down the world's y axis: no
    # camera of the ring, nor the planted one or ROVER, has a Gaussian on its y axis inside its image
    vms[Y_CAM] = pc.look_at((0.25, -3.0, 0.125), (0.25, -2.0, 0.125))
    return vms, Ks


def campos_of(viewmats):
    from oracle import gs_oracle as go
    return go.camera_positions(viewmats)


_cases = {}


def get(N, Cn):
    """the project_cases.Case of N Gaussians and Cn cameras, sh [N, 16, 3] (every degree reads its own rows of it), with
    tags: axis, plane, close, culled (lists of Gaussian indices), and .vis [Cn, N] (the oracle's)"""
    if (N, Cn) in _cases:
        return _cases[(N, Cn)]
    s = pc.Soup(900 + 10 * Cn + N % 97)
    rng = s.rng
    vms, Ks = cameras(Cn)
    cp = campos_of(vms).astype(np.float64)
    tags = dict(axis=[], plane=[], close=[], culled=[])
    planted = []
    if Cn <= 2:
        planted += [("axis", (0.0, 0.0, 2.0), 0.1), ("plane", (0.0, 0.5, 2.0), 0.1), ("plane", (-0.5, 0.0, 2.0), 0.1)]
    else:
        # (the float32 camera positions the kernels are given, one coordinate moved: the other two differences are 0.0)
        planted += [("axis", tuple(cp[0] + np.array([-3.0, 0.0, 0.0])), 0.1),
                    ("axis", tuple(cp[Y_CAM] + np.array([0.0, 3.0, 0.0])), 0.1)]
    fwd = vms[-1][2, :3].astype(np.float64)                        # the last camera's viewing direction in the world
    planted += [("close", tuple(cp[-1] + 1e-3 * fwd), 1e-6)]
    for tag, mean, scale in planted[:N]:
        tags[tag].append(s.add(mean, scale))
    n_rest = N - len(s.m)
    if Cn <= 2:
        s.ordinary(n_rest, xr=(-0.9, 1.1), yr=(-0.7, 1.1))   # (wider than the image: some are inside one camera only)
    else:
        pc._cloud(s, n_rest)
    case = s.case("sh_n%d_c%d" % (N, Cn), W, H, vms, Ks, None, near=NEAR)
    case.vis = pc.oracle_forward(case)["vis"].reshape(Cn, N)
    tags["culled"] = [g for g in range(N) if case.vis[:, g].any() and not case.vis[:, g].all() and g not in tags["close"]][:2]
    # coefficients: 16 rows; g % 4 channels pushed under the clamp by their DC term, one Gaussian in eight left to the view
    k = rng.uniform(-0.3, 0.3, (N, 16, 3))
    for g in range(N):
        for tries in range(1000):
            k[g] = rng.uniform(-0.3, 0.3, (16, 3))
            dc = rng.uniform(1.0, 6.0, 3) * np.where(np.arange(3) < g % 4, -1.0, 1.0)
            k[g, 0] = rng.permutation(dc) if g % 8 != 7 else rng.uniform(-2.2, -1.4, 3)
            kf = k[g:g + 1].astype(np.float32)
            ok = True
            for deg in DEGREES:
                p = pre_clamp(case.means[g:g + 1], cp.astype(np.float32), kf, deg)[:, 0]
                ok &= bool((np.abs(p[case.vis[:, g]]) >= MARGIN).all())
            if ok:
                break
        assert ok
    case.sh = np.ascontiguousarray(k, np.float32)
    case.tags = tags
    _cases[(N, Cn)] = case
    return case


def colour_cotangents(case, seed=5):
    """v_splats [Cn * N, 12]: standard normal on the colour columns 6:9 of the visible pairs, 0 on their other columns (the
    means block of the backward is then the direction term alone), NaN in all twelve floats of every culled pair"""
    v = np.zeros((case.Cn * case.N, 12), np.float32)
    v[:, 6:9] = np.random.default_rng(seed).standard_normal((case.Cn * case.N, 3)).astype(np.float32)
    v[~case.vis.reshape(-1)] = np.nan
    return v


# ---------------------------------------------------------------------------------------------------------------------
# references
def ref64(case, deg, v_splats):
    """float64 torch autograd of sum(colour * cotangent) over the visible pairs: dict sh [N, K, 3], means [N, 3],
    viewmats [Cn, 4, 4] (through campos = inverse(V)[:3, 3]), and colour [Cn, N, 3]"""
    import torch
    N, Cn, K = case.N, case.Cn, rows(deg)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    means, sh, vm = t(case.means).requires_grad_(), t(case.sh[:, :K]).requires_grad_(), t(case.viewmats).requires_grad_()
    # the VALUE of the float32 camera positions the kernels are given (1e-3 from a centre, a float64 inverse is another
    # direction), the derivative of inverse(V)[:3, 3]
    campos = torch.inverse(vm)[:, :3, 3]
    campos = campos + (t(campos_of(case.viewmats)) - campos).detach()
    d = means[None] - campos[:, None]
    u = d / d.norm(dim=-1, keepdim=True)
    b = torch.stack(basis(u[..., 0], u[..., 1], u[..., 2], deg))
    col = torch.clamp_min(torch.einsum("kcn,nkj->cnj", b, sh) + 0.5, 0.0)
    vis = torch.tensor(case.vis)
    vc = t(np.nan_to_num(np.asarray(v_splats, np.float64)).reshape(Cn, N, 12)[..., 6:9])
    loss = (col * vc)[vis].sum()
    G = torch.autograd.grad(loss, [sh, means, vm], allow_unused=True)
    out = {k: (np.zeros(tuple(p.shape)) if g is None else g.numpy()) for k, g, p in zip(GROUPS, G, (sh, means, vm))}
    out["colour"] = col.detach().numpy()
    return out


def restate(case, deg, v_splats, dtype=np.float32):
    """the kernels' chain rule, written out in numpy in `dtype` (the camera sums in dtype, in camera order; the pose
    gradient's sums and finish in float64, as k_viewmat_bwd_part / _finish hold them): the same dict as ref64"""
    N, Cn, K = case.N, case.Cn, rows(deg)
    campos = campos_of(case.viewmats)
    u, inrm = directions(case.means, campos, dtype)
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    b = np.stack(basis(x, y, z, deg)).astype(dtype)
    k = case.sh[:, :K].astype(dtype)
    pre = np.einsum("kcn,nkj->cnj", b, k).astype(dtype) + dtype(0.5)
    vc = np.nan_to_num(np.asarray(v_splats, dtype)).reshape(Cn, N, 12)[..., 6:9]
    vc = np.where((pre >= 0) & case.vis[..., None], vc, dtype(0)).astype(dtype)
    v_k = np.zeros((N, K, 3), dtype)
    v_m = np.zeros((N, 3), dtype)
    v_campos = np.zeros((Cn, 3), np.float64)
    db = basis_grad(x, y, z, deg)
    for c in range(Cn):
        v_k += (b[:, c, :, None] * vc[None, c]).transpose(1, 0, 2).astype(dtype)
        tt = np.einsum("nkj,nj->kn", k, vc[c]).astype(dtype)                              # [K, N]
        vu = np.zeros((N, 3), dtype)
        for i in range(K):
            for a in range(3):
                vu[:, a] += (np.asarray(db[i][a], dtype)[c] * tt[i]).astype(dtype)
        dot = (vu * u[c]).sum(-1, keepdims=True).astype(dtype)
        v_d = ((vu - dot * u[c]) * inrm[c][:, None]).astype(dtype)
        v_m += v_d
        v_campos[c] = -v_d.astype(np.float64).sum(0)
    inv = np.linalg.inv(case.viewmats.astype(np.float64))
    v_vm = np.zeros((Cn, 4, 4))
    for c in range(Cn):
        v_vm[c] = -np.outer(inv[c][:3, :].T @ v_campos[c], inv[c][:, 3])
    return dict(sh=v_k, means=v_m, viewmats=v_vm, colour=np.where(case.vis[..., None], np.maximum(pre, 0), 0))


def bounds(o32, r64):
    """per group, as project_cases.grad_bounds: rel = 4 x the worst relative error of the float32 restatement against
    float64 -- per Gaussian (per camera for viewmats), relative to its own largest entry floored at FLOOR x the group's
    -- floored at FLOOR; and the scales"""
    out = {}
    for g in GROUPS:
        n = r64[g].shape[0]
        a, r = np.asarray(o32[g], np.float64).reshape(n, -1), r64[g].reshape(n, -1)
        own = np.abs(r).max(1)
        scale = np.maximum(own, FLOOR * max(float(own.max()), 1e-300))
        worst = float((np.abs(a - r).max(1) / scale).max())
        out[g] = dict(rel=max(4.0 * worst, FLOOR), own=worst, scale=scale)
    return out


def excess(got, r64, bnd, group):
    """the worst error of `got` in units of the group's bound (<= 1 passes)"""
    n = r64[group].shape[0]
    err = np.abs(np.asarray(got, np.float64).reshape(n, -1) - r64[group].reshape(n, -1)).max(1)
    return float((err / (bnd[group]["scale"] * bnd[group]["rel"])).max())


_refs = {}


def reference(N, Cn, deg):
    """computed once per (N, Cn, deg) and shared, never modified: case, v (cotangents), r64, o32, bounds"""
    key = (N, Cn, deg)
    if key not in _refs:
        case = get(N, Cn)
        v = colour_cotangents(case)
        r64, o32 = ref64(case, deg, v), restate(case, deg, v)
        _refs[key] = dict(case=case, v=v, r64=r64, o32=o32, bounds=bounds(o32, r64))
    return _refs[key]


def clamped_counts(case, deg):
    """set of the numbers of clamped channels over the visible pairs"""
    p = pre_clamp(case.means, campos_of(case.viewmats), case.sh, deg)
    return set(np.unique((p < 0).sum(-1)[case.vis]).tolist())
