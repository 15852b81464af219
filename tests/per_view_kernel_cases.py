"""Hand-built inputs that plant the edges of the per-view kernels -- everything behind per_view.h: k_viewmat_bwd_part /
k_viewmat_bwd_finish (gs_pose_bwd.hip), k_intrinsics_bwd_part (gs_intrinsics.hip), k_exposure_fwd / k_exposure_bwd
(gs_exposure.hip), k_dprior_loss (loss_depth.hip), k_weight_sums and k_stream_finish (per_view.h) and the three per-view
Adam kernels (numpy; torch for the float64 references; no GPU).

Used by test_oracle_per_view_cases.py (CPU: every case reaches the edge it names, the numpy oracle of
oracle/per_view_oracle.py IS the operation, the bounds) and test_gpu_per_view_cases.py (the kernels).
tests/per_view_cases.py -- the helpers of the per-view FEATURE tests -- is another file and stays as it is.

a. PAIR CASES.  Every case of project_cases.CASES (the cull, clamp, colour-clamp, view-count, tail and SH-stride edges that
were planted for k_project_sh_bwd: the two per-view kernels hold copies of its per-pair arithmetic) and six of their own:

    n0             N = 0: no partials, the finishers alone; exact +0.0 in all 16 + 4 entries
    trip2          256 * 256 + 1 Gaussians, one camera: 257 partials -- the finishers' strided loop wraps with exactly one
                   element in its second trip; live pairs in block 0, in block 255 and ALONE in block 256
    similarity_V   V = [1.25 R  t; 0 0 0 1]: the finisher's general 4 x 4 inverse off the rigid matrices
    general_row3   bottom row (0.01, -0.02, 0.03, 1.1): the projection ignores it, inverse(V) does not
    cancel         one camera, 32 Gaussians and their mirror images through the optical axis with v_means2d of the
                   opposite sign: v_t.x, v_t.y, v_cx, v_cy are sums of cancelling terms (why the kernels sum in double)
    dead_camera    three cameras, the middle one sees nothing: its rows are exact zeros, its neighbours' unchanged

The kernels read the splat records of the float32 C oracle (project_cases.oracle_forward), with NaN in every float of a
culled record but the radius word, and the cotangents of project_cases.cotangents (NaN on every culled pair).

The yardstick is PER ENTRY.  S = sum over the camera's pairs of |float64 contribution| (for the pose pushed through the
finisher with absolute values: |base| + sum |inv| S_campos |w|); own32 = max over the case's cameras and entries of
|float32 oracle - float64| / S; the kernel's bound on an entry is 4 max(own32 of the case, median own32 over all cases) S
(the factor: project_cases.grad_bounds).  Measured own32 (this file's inputs, numpy float32 against float64 autograd;
test_oracle_per_view_cases.test_bounds_come_from_the_float32_oracle prints this table and holds it to what it measures),
and "new/old": the entry's bound over the old bar, 1e-6 of the camera's largest entry, at its largest over the small
entries (below a tenth of the camera's largest) / over the others -- above 1 where S exceeds the largest entry, i.e.
where the entry's terms cancel ("Per-view kernels on every pair, sum, stream and Adam edge"):

    case               pose      intrinsics pose new/old     intrinsics new/old
    near_far           2.1e-07   4.6e-08    1.42 / 2.22      0.40 / 0.49
    screen_edges       4.9e-08   2.9e-08    0.49 / 1.56      0.38 / 0.71
    radius_clip_eq     1.3e-07   9.1e-08    0.04 / 0.54      0.00 / 0.36
    radius_clip_below  1.3e-07   7.3e-08    0.06 / 0.55      0.00 / 0.34
    det_zero_eps0      7.1e-07   1.1e-07    9.67 / 17.83     0.32 / 3.17
    det_zero_eps03     1.7e-07   3.4e-08    5.17 / 2.57      1.19 / 1.26
    clamp_xp           2.9e-08   8.4e-09    1.82 / 2.67      2.23 / 1.64
    clamp_xn           6.6e-08   4.1e-08    1.34 / 1.96      0.13 / 4.43
    clamp_yp           6.7e-08   2.2e-08    2.89 / 4.24      0.00 / 3.39
    clamp_yn           5.5e-08   2.2e-08    2.01 / 2.95      0.98 / 0.72
    quat_norm          1.3e-07   3.5e-08    3.11 / 5.11      0.00 / 1.07
    colour_clamp       2.2e-07   3.6e-08    4.36 / 6.40      1.90 / 1.40
    mixed_visibility   9.4e-08   7.8e-08    0.44 / 1.38      0.08 / 1.00
    views_c1           4.0e-08   2.0e-08    1.12 / 3.87      0.32 / 2.17
    views_c8           5.5e-08   3.0e-08    2.14 / 3.84      0.29 / 3.04
    views_c9           6.4e-08   4.3e-08    2.31 / 3.81      0.42 / 4.22
    views_c64          1.6e-07   4.7e-08    6.88 / 9.20      3.08 / 5.75
    views_c256         2.2e-07   5.2e-08    12.57 / 16.05    3.41 / 8.83
    tails_n1           8.6e-07   1.8e-07    0.14 / 3.44      0.00 / 0.71
    tails_n63          6.6e-08   2.5e-08    0.89 / 3.10      0.00 / 3.67
    tails_n64          5.4e-08   2.0e-08    1.16 / 1.47      0.38 / 2.12
    tails_n65          7.5e-08   1.9e-08    0.91 / 1.61      1.45 / 2.01
    tails_n255         2.3e-08   9.5e-09    1.34 / 3.46      0.00 / 3.13
    tails_n256         3.6e-08   8.3e-09    1.59 / 3.77      0.21 / 2.28
    tails_n257         2.0e-08   9.0e-09    0.77 / 4.99      0.00 / 2.27
    sh_stride_12       4.4e-08   1.7e-08    2.22 / 4.04      0.00 / 1.53
    sh_stride_72       4.4e-08   1.7e-08    2.22 / 4.04      0.00 / 1.53
    regulariser_n257   3.7e-08   2.7e-08    1.30 / 4.91      0.00 / 2.38
    regulariser_n1000  4.4e-08   2.1e-08    1.46 / 5.47      0.00 / 2.67
    n0                 0.0e+00   0.0e+00    -                -
    trip2              5.9e-08   5.9e-08    0.16 / 0.68      0.16 / 0.72
    similarity_V       4.5e-08   3.1e-08    0.85 / 2.68      2.31 / 1.70
    general_row3       8.2e-08   3.6e-08    1.13 / 3.52      2.69 / 1.97
    cancel             8.4e-08   4.2e-08    3.63 / 5.05      2.83 / 0.41
    dead_camera        4.4e-08   5.2e-08    0.81 / 1.40      0.89 / 5.61
    median             6.4e-08   3.1e-08

b. STREAM SHAPES: STREAM_SHAPES, each tagged by oracle.per_view_oracle.stream_tags (computed, not typed in); dyadic inputs,
so that every double sum is exact in any order and the kernels are compared with ==.

c. ADAM CASES: adam_case() for the three kernels.
"""
import numpy as np

import project_cases as pc
from oracle import per_view_oracle as pvo

FLOOR = pc.FLOOR

# ---------------------------------------------------------------------------------------------------------------------
# a. pair cases
TRIP2_N = 256 * 256 + 1


def _to_world(V, p):
    """world point whose camera coordinates under the rigid V are p"""
    R, t = V[:3, :3].astype(np.float64), V[:3, 3].astype(np.float64)
    return R.T @ (np.asarray(p, np.float64) - t)


def n0():
    W, H = 80, 48
    vm, Ks = pc.two_cams(W, H)
    z = lambda *s: np.zeros(s, np.float32)

    def check(case, O):
        assert case.N == 0 and case.Cn == 2 and O["records"].shape == (0, 12)
    return pc.Case("n0", W, H, z(0, 3), z(0, 4), z(0, 3), z(0), z(0, 4, 3), vm, Ks, check)


TRIP2_LIVE = (0, 1, 63, 64, 255, 256, 300, 32767, 32768, 65279, 65280, 65281, 65343, 65344, 65535, 65536)


def trip2():
    W, H = 80, 48
    N = TRIP2_N
    s = pc.Soup(90)
    s.ordinary(len(TRIP2_LIVE), xr=(-0.35, 0.35), yr=(-0.3, 0.3))
    V = pc.ROVER
    means = np.tile(np.array([0.0, 0.0, -5.0]), (N, 1))                  # behind the camera: culled by z < near
    quats = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
    scales = np.full((N, 3), 0.1); opac = np.full(N, 0.5); sh = np.zeros((N, 4, 3))
    for n, i in enumerate(TRIP2_LIVE):
        means[i] = _to_world(V, s.m[n]); quats[i] = s.q[n]; scales[i] = s.s[n]; opac[i] = s.o[n]; sh[i] = s.k[n]

    def check(case, O):
        assert case.N == 256 * 256 + 1 and case.Cn == 1 and -(-case.N // 256) == 257
        live = np.nonzero(O["vis"])[0]
        assert live.tolist() == sorted(TRIP2_LIVE)
        blocks = live // 256
        assert (blocks == 0).sum() >= 4 and (blocks == 255).sum() >= 4 and (blocks == 256).sum() == 1
        assert live[-1] == 65536 and 65536 % 256 == 0                # alone: thread 0 of the 257th block
    return pc.Case("trip2", W, H, means, quats, scales, opac, sh, V[None], pc.rover_K(W, H)[None], check)


def _two_special(name, V0):
    W, H = 80, 48
    s = pc.Soup(91)
    s.ordinary(24, xr=(-0.3, 0.4), yr=(-0.3, 0.4))
    vm = np.stack([V0, pc.viewmat()]); Ks = np.stack([pc.rover_K(W, H), pc.planted_K(W, H)])

    def check(case, O):
        vis = O["vis"].reshape(case.Cn, case.N)
        assert vis[0].sum() >= 12
        V = case.viewmats[0].astype(np.float64)
        inv = np.linalg.inv(V)
        Rt = V[:3, :3] @ V[:3, :3].T
        if name == "similarity_V":
            assert np.allclose(Rt, 1.5625 * np.eye(3), atol=1e-6) and V[3].tolist() == [0, 0, 0, 1]
            assert np.abs(inv[:3, :3] - V[:3, :3].T).max() > 0.05    # inverse(V) is not [R^T, -R^T t]
        else:
            assert np.allclose(V[3], [0.01, -0.02, 0.03, 1.1], atol=1e-7)
            assert np.abs(inv[3, :3]).min() > 1e-3 and abs(inv[3, 3] - 1.0) > 0.05       # a bottom row of its own
    return s.case(name, W, H, vm, Ks, check)


def similarity_V():
    V = pc.ROVER.copy()
    V[:3, :3] *= np.float32(1.25)
    return _two_special("similarity_V", V)


def general_row3():
    V = pc.ROVER.copy()
    V[3] = np.array([0.01, -0.02, 0.03, 1.1], np.float32)
    return _two_special("general_row3", V)


CANCEL_PAIRS = 32


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def cancel():
    """Gaussian 2 i + 1 is Gaussian 2 i turned by 180 degrees about the optical axis of the (one, turned and moved) camera:
    camera coordinates (-x, -y, z), camera covariance F S F with F = diag(-1, -1, 1), hence the same cov2d and conic, and
    J' = -J F.  Its cotangents (cancel_cotangents): v_means2d' = -(1 + delta) v_means2d, v_conic' = v_conic; then
    v_p.x' = -v_p.x, v_p.y' = -v_p.y up to delta and float32 rounding of the mirror image."""
    W, H = 80, 48
    V = pc.ROVER
    s = pc.Soup(92)
    base = s.ordinary(CANCEL_PAIRS, xr=(-0.3, 0.3), yr=(-0.25, 0.25))
    R = V[:3, :3].astype(np.float64)
    axis = R.T @ np.array([0.0, 0.0, 1.0])
    qF = np.array([0.0, axis[0], axis[1], axis[2]])                      # 180 degrees about the optical axis, world frame
    m, q, sc, o, k = [], [], [], [], []
    for i in base:
        p = s.m[i]
        for twin in (False, True):
            m.append(_to_world(V, (-p[0], -p[1], p[2]) if twin else p))
            q.append(_qmul(qF, s.q[i]) if twin else s.q[i])
            sc.append(s.s[i]); o.append(s.o[i]); k.append(s.k[i])

    def check(case, O):
        assert case.N == 2 * CANCEL_PAIRS and case.Cn == 1 and O["vis"].all()
        p = case.cam_coords()[0]
        assert np.allclose(p[0::2, :2], -p[1::2, :2], atol=1e-6) and np.allclose(p[0::2, 2], p[1::2, 2], atol=1e-6)
        assert np.allclose(O["records"][0::2, 3:6], O["records"][1::2, 3:6], rtol=1e-4)
        sides, _ = pc.clamp_sides(case, O)
        assert not any(v.any() for v in sides.values())              # nothing clamped: v_cx is the plain sum of v_means2d.x
    return pc.Case("cancel", W, H, np.array(m), np.array(q), np.array(sc), np.array(o), np.array(k), V[None],
                   pc.rover_K(W, H)[None], check)


def cancel_cotangents(case, vis):
    v = pc.cotangents(case, vis, seed=6)
    delta = np.where(np.arange(CANCEL_PAIRS) % 2 == 0, 2.0 ** -12, 0.0).astype(np.float32)
    v[1::2, 0:2] = -(1.0 + delta)[:, None] * v[0::2, 0:2]
    v[1::2, 3:6] = v[0::2, 3:6]
    return v


def dead_camera():
    W, H = 80, 48
    s = pc.Soup(93)
    s.ordinary(24)
    away = pc.look_at((0.0, 0.0, 0.0), (0.1, 0.0, -5.0))                 # every Gaussian (z >= 1) is behind it
    vm = np.stack([pc.viewmat(), away, pc.ROVER])
    Ks = np.stack([pc.planted_K(W, H), pc.intr(40.0, 64.0, 46.0, 20.0), pc.rover_K(W, H)])

    def check(case, O):
        vis = O["vis"].reshape(case.Cn, case.N)
        assert not vis[1].any() and vis[0].sum() >= 12 and vis[2].sum() >= 12
    return s.case("dead_camera", W, H, vm, Ks, check)


NEW_CASES = {"n0": n0, "trip2": trip2, "similarity_V": similarity_V, "general_row3": general_row3, "cancel": cancel,
             "dead_camera": dead_camera}
PAIR_CASES = list(pc.CASES) + list(NEW_CASES)

# A case whose relative bound 4 max(own32, median) may exceed FLOOR says so here, with the reason (none does without one)
ABOVE_FLOOR = {
    "pose": {},
    "intrinsics": {},
}

_cases = {}


def get(name):
    if name in pc.CASES:
        return pc.get(name)
    if name not in _cases:
        _cases[name] = NEW_CASES[name]()
    return _cases[name]


def nan_culled(records, vis):
    """a copy of the records with NaN in every float of a culled record but the radius word (float 10: integer 0) -- the
    kernels test the radius word first and load nothing else of a culled pair"""
    rec = np.array(records, np.float32, copy=True)
    dead = ~np.asarray(vis, bool)
    keep = rec[dead, 10].copy()
    rec[dead] = np.nan
    rec[dead, 10] = keep
    return rec


_refs = {}


def pair_reference(name):
    """computed once per case and shared, never modified: case, vis, records (NaN on culled), v (cotangents, NaN on
    culled), cam (camera of every visible pair, flat order) and per kernel ("pose": [Cn, 4, 4]; "intrinsics": [Cn, 4])
    r64 (float64 autograd), t64 (finisher of the float64 pair terms), o32 (finisher of the double sum of the float32 pair
    terms), S (entry scale), own32"""
    if name in _refs:
        return _refs[name]
    case = get(name)
    Cn, N = case.Cn, case.N
    if N == 0:
        O = dict(vis=np.zeros(0, bool), records=np.zeros((0, 12), np.float32))
    else:
        O = pc.reference(name)["O"] if name in pc.CASES else pc.oracle_forward(case)
    vis = O["vis"]
    rec = nan_culled(O["records"], vis)
    if name in pc.CASES:
        v = pc.reference(name)["v"]
    elif name == "cancel":
        v = cancel_cotangents(case, vis)
    else:
        v = pc.cotangents(case, vis)
    if N == 0:
        r64 = dict(viewmats=np.zeros((Cn, 4, 4)), Ks4=np.zeros((Cn, 4)))
    else:
        r64 = pc.ref64(case, vis, v, reg=False, cameras=True)
    _, cam, _ = pvo.visible_pairs(rec, N)
    out = dict(case=case, O=O, vis=vis, records=rec, v=v, cam=cam)
    V = case.viewmats.astype(np.float64)
    for kind, terms, ref in (("pose", pvo.pose_pair_terms, r64["viewmats"]), ("intrinsics", pvo.intrinsics_pair_terms, r64["Ks4"])):
        t32, t64 = terms(case, rec, v, np.float32), terms(case, rec, v, np.float64)
        s32, s64, sab = pvo.camera_sums(t32, cam, Cn), pvo.camera_sums(t64, cam, Cn), pvo.camera_sums(t64, cam, Cn, True)
        if kind == "pose":
            o32 = np.stack([pvo.pose_finish(s32[c], V[c]) for c in range(Cn)])
            f64 = np.stack([pvo.pose_finish(s64[c], V[c]) for c in range(Cn)])
            S = np.stack([pvo.pose_finish(sab[c], V[c], absolute=True) for c in range(Cn)])
        else:
            o32, f64, S = pvo.intrinsics_finish(s32), pvo.intrinsics_finish(s64), sab
        err = np.abs(o32 - ref)
        own = float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
        out[kind] = dict(r64=np.asarray(ref, np.float64), t64=f64, o32=o32, S=S, own32=own, sums64=s64, sums_abs=sab)
    _refs[name] = out
    return out


_rel = {}


def rel_bounds(kind):
    """{case: 4 max(own32 of the case, median own32 over all cases)} for kind = "pose" / "intrinsics"; the median keeps a case
    whose float32 error happens to vanish (n0, a camera at the origin ...) from demanding the impossible"""
    if kind not in _rel:
        own = {n: pair_reference(n)[kind]["own32"] for n in PAIR_CASES}
        med = float(np.median(list(own.values())))
        _rel[kind] = {n: 4.0 * max(o, med) for n, o in own.items()}
        _rel[kind + "_median"] = med
    return _rel[kind]


# ---------------------------------------------------------------------------------------------------------------------
# b. stream shapes
STREAM_SHAPES = [(1, 45, 23), (2, 33, 63), (3, 33, 32), (1, 1, 1028), (8, 120, 160), (256, 4, 4), (1, 257, 1024),
                 (1, 2049, 1024)]
EXPOSURE_SHAPES = STREAM_SHAPES[:-1]        # (exposure has (3, 768, 1024) for the cap: test_gpu_exposure)


def shape_tags(shape, aligned=True):
    C, H, W = shape
    return pvo.stream_tags(C, H * W, aligned)


def exposure_inputs(shape, seed=0):
    """x in [0, 1] multiples of 1/16, v_y in [-2, 2] multiples of 1/8, E = [A | t] multiples of 1/8 in [-2, 2]: y and v_x are
    sums of at most four terms that are multiples of 1/128 and 1/64 below 8 and 12 -- exact in float32, fused or not;
    every product v_y x is a multiple of 1/128 below 2, so a double sum of up to 2^40 of them is exact in any order"""
    C, H, W = shape
    rng = np.random.default_rng(700 + seed + 13 * C + H * W)
    x = (rng.integers(0, 17, (C, H, W, 3)) / 16.0).astype(np.float32)
    vy = (rng.integers(-16, 17, (C, H, W, 3)) / 8.0).astype(np.float32)
    E = (rng.integers(-16, 17, (C, 3, 4)) / 8.0).astype(np.float32)
    return x, vy, E


def exposure_reference(x, vy, E):
    """float64: y, v_x [C,H,W,3] and v_E [C,3,4] (before its float32 rounding)"""
    x, vy, E = (np.asarray(a, np.float64) for a in (x, vy, E))
    A, t = E[:, :, :3], E[:, :, 3]
    y = np.einsum("cji,chwi->chwj", A, x) + t[:, None, None, :]
    vx = np.einsum("cji,chwj->chwi", A, vy)
    vE = np.concatenate([np.einsum("chwj,chwi->cji", vy, x), vy.sum((1, 2))[:, :, None]], 2)
    return y, vx, vE


DP_MIN_ALPHA = np.float32(1e-10)
DEPTH_FAC = 0.75


def depth_inputs(shape, seed=0):
    """alpha in {1, 0.5, 0.25, 0, 5e-11}; D, Z multiples of 1/16 in [0, 4); w multiples of 1/8 in [0, 2] with holes (0),
    NaN and negative weights; Z is NaN or inf wherever w <= 0 or w is NaN; where alpha < 1e-10, D is 0 except on up to eight
    weighted pixels per view (D = 1/16: ED = 6.25e8, a float32 whose unit is 64 -- the sum stays within 53 bits); on every
    11th weighted pixel of alpha 1, Z = D: an exact tie.  With more than one view the last has no weight at all."""
    C, H, W = shape
    rng = np.random.default_rng(800 + seed + 13 * C + H * W)
    n = (C, H, W)
    alpha = rng.choice(np.array([1.0, 0.5, 0.25, 0.0, 5e-11], np.float32), n, p=[0.4, 0.25, 0.25, 0.05, 0.05])
    D = (rng.integers(0, 64, n) / 16.0).astype(np.float32)
    Z = (rng.integers(0, 64, n) / 16.0).astype(np.float32)
    w = (rng.integers(1, 17, n) / 8.0).astype(np.float32)
    u = rng.uniform(0, 1, n)
    w[u < 0.25] = 0.0
    w[(u >= 0.25) & (u < 0.28)] *= -1.0
    w[(u >= 0.28) & (u < 0.30)] = np.nan
    if C > 1:
        w[C - 1] = np.where(w[C - 1] > 0, 0.0, w[C - 1])
    on = w > 0
    low = alpha < DP_MIN_ALPHA
    D[low] = 0.0
    for c in range(C):
        idx = np.flatnonzero(low[c] & on[c])[:8]
        D[c].reshape(-1)[idx] = 1.0 / 16.0
    tie = np.zeros(n, bool)
    for c in range(C):
        idx = np.flatnonzero((alpha[c] == 1.0) & on[c])[::11]
        tie[c].reshape(-1)[idx] = True
    Z[tie] = D[tie]
    off = ~on
    Z[off] = np.where(rng.integers(0, 2, int(off.sum())) == 0, np.nan, np.inf).astype(np.float32)
    return D, alpha, Z, w, tie


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def depth_reference(D, alpha, Z, w, depth_fac=DEPTH_FAC):
    """float64, rounded to float32 where loss_depth.hip rounds (a product of two float32 is exact in double and a quotient of
    two float32 rounds to float32 the same through double): sums [C] = sum_p w |ED - Z|, n_c [C], v_depth, v_alpha, ED"""
    D, alpha, Z, w = (np.asarray(a, np.float32) for a in (D, alpha, Z, w))
    on = w > 0
    w64 = np.where(on, w, 0.0).astype(np.float64)
    n_c = np.maximum(w64.sum((1, 2)), 1.0)
    k = _r32(depth_fac / n_c)[:, None, None]
    ac = np.maximum(alpha, DP_MIN_ALPHA).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ed = _r32(D.astype(np.float64) / ac)
        diff = np.where(on, ed - np.where(on, Z, 0.0).astype(np.float64), 0.0)
        g = _r32(_r32(k * w64) * np.sign(diff))
        v_d = np.where(on, _r32(g / ac), 0.0)
        v_a = np.where(on & (alpha >= DP_MIN_ALPHA), _r32(-_r32(g * ed) / ac), 0.0)
    terms = w64 * np.abs(diff)
    return dict(sums=terms.sum((1, 2)), n_c=n_c, v_depth=v_d, v_alpha=v_a, ed=ed, terms=terms, w64=w64)


def weight_sums_reference(w):
    """(n1, n2) [C] of loss_l1_ssim_weighted: max(sum_p w, 1) and the same over the interior, 5 pixels from every edge;
    the weights that count are w > 0"""
    w = np.asarray(w, np.float32)
    w64 = np.where(w > 0, w, 0.0).astype(np.float64)
    H, W = w.shape[1:]
    inner = w64[:, 5:H - 5, 5:W - 5] if H > 10 and W > 10 else np.zeros((w.shape[0], 0, 0))
    return np.maximum(w64.sum((1, 2)), 1.0), np.maximum(inner.sum((1, 2)), 1.0), w64


# ---------------------------------------------------------------------------------------------------------------------
# c. Adam cases
ADAM_C = (1, 63, 64, 65)
ADAM_BETAS = ((0.9, 0.999), (0.0, 0.0), (0.5, 0.9))
ADAM_STEPS = (1, 2, 100000)
ADAM_EPS = 1e-8
ADAM_W, ADAM_H = 64, 32                     # the image of the intrinsics cases: powers of two, so W v_cx is exact
MASK_PATTERN = (1.0, 0.0, -0.0, 1e-30)      # -0.0 freezes a view (mask == 0), 1e-30 does not


def adam_mask(C):
    return np.array([MASK_PATTERN[c % 4] for c in range(C)], np.float32)


def zero_view(C):
    """the live view with zero gradient and zero moments (mask 1 or 1e-30)"""
    return 0 if C < 4 else 4


def adam_case(kind, C, betas, step, seed=0, zero_moments=False):
    """kind "exposure" (12 scalars per view), "intrinsics" (4), "pose" (6; gradient [C,4,4]).  -> dict: mask [C], param,
    grad, m, v (float32), zero (the zero view, on step-1 cases: zero gradient and zero moments), frozen [C] bool.
    Frozen views carry -0.0 in a moment and in a gradient entry: every bit must come back."""
    nv = dict(exposure=12, intrinsics=4, pose=6)[kind]
    rng = np.random.default_rng(900 + seed + 7 * C + 31 * step % 1000 + int(1000 * betas[0]))
    mask = adam_mask(C)
    m = (0.01 * rng.standard_normal((C, nv))).astype(np.float32)
    v = (1e-4 * rng.uniform(0.0, 1.0, (C, nv))).astype(np.float32)
    if zero_moments:
        m[:] = 0.0; v[:] = 0.0
    if kind == "exposure":
        param = (np.tile(np.eye(3, 4), (C, 1, 1)) + 0.1 * rng.standard_normal((C, 3, 4))).astype(np.float32)
        grad = rng.standard_normal((C, 3, 4)).astype(np.float32)
    elif kind == "intrinsics":
        param = np.stack([pc.intr(rng.uniform(40, 90), rng.uniform(40, 90), rng.uniform(20, 60), rng.uniform(10, 40))
                          for _ in range(C)])
        grad = (1e-2 * rng.standard_normal((C, 4))).astype(np.float32)
    else:
        param = np.stack([pc.viewmat(pc.rot(*rng.uniform(-1.0, 1.0, 3)), rng.uniform(-2.0, 2.0, 3)) for _ in range(C)])
        grad = rng.standard_normal((C, 4, 4)).astype(np.float32)     # row 3 too: the kernel must ignore it
    frozen = mask == 0
    z = None
    if step == 1:
        z = zero_view(C)
        assert not frozen[z]
        grad[z] = 0.0; m[z] = 0.0; v[z] = 0.0
    # PLANTED: slot nv - 1 of every view: g = -9 m exactly (m of 16 bits; for the intrinsics g = H v_cy with H a power of two).
    # With beta1 = 0.9 the two products b1 m and (1 - b1) g cancel to 2e-16 m, the size of their own double roundings: which
    # of the two is rounded and which is fused (M_LAST of per_view_adam_delta) then shows in the leading bits of the stored
    # float32 moment -- on random inputs it shows in one stored moment of several thousand
    planted = np.zeros((C, nv), bool)
    if kind != "pose":
        m[:, nv - 1] = np.round(m[:, nv - 1] * 2.0 ** 22) / 2.0 ** 22
        gp = (-9.0 * m[:, nv - 1].astype(np.float64)) / (ADAM_H if kind == "intrinsics" else 1.0)
        grad.reshape(C, -1)[:, -1] = gp.astype(np.float32)
        assert np.array_equal(grad.reshape(C, -1)[:, -1].astype(np.float64), gp)
        planted[:, nv - 1] = True
    if z is not None:
        grad[z] = 0.0; m[z] = 0.0; v[z] = 0.0
        planted[z] = False
    m[frozen, 0] = -0.0
    grad.reshape(C, -1)[frozen, 1] = -0.0
    planted[frozen] = False
    return dict(planted=planted, kind=kind, C=C, betas=betas, step=step, mask=mask, param=param, grad=grad, m=m, v=v, zero=z, frozen=frozen)


def _hat(w):
    import torch
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def ref_pose_step(V, G, m, v, lr, b1, b2, eps, step):
    """the update rule of gs_pose_step.hip in float64 torch, the retraction through matrix_exp: V [C,4,4], G [C,4,4], m, v
    [C,6] (numpy) -> V', campos', m', v', delta (numpy float64)"""
    import torch
    V, G, m, v = (torch.tensor(np.asarray(a, np.float64)) for a in (V, G, m, v))
    R, t = V[:, :3, :3], V[:, :3, 3]
    GR, Gt = G[:, :3, :3], G[:, :3, 3]
    A = GR @ R.transpose(1, 2)
    g_om = torch.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], -1) + \
        torch.linalg.cross(t, Gt)
    g = torch.cat([g_om, Gt], -1)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    delta = -lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    E = torch.linalg.matrix_exp(_hat(delta[:, :3]))
    Rn = E @ R
    tn = (E @ t[:, :, None])[:, :, 0] + delta[:, 3:]
    r0 = Rn[:, 0] / Rn[:, 0].norm(dim=-1, keepdim=True)
    r1 = Rn[:, 1] - (Rn[:, 1] * r0).sum(-1, keepdim=True) * r0
    r1 = r1 / r1.norm(dim=-1, keepdim=True)
    r2 = torch.linalg.cross(r0, r1)
    Rn = torch.stack([r0, r1, r2], 1)
    Vn = torch.zeros_like(V)
    Vn[:, :3, :3] = Rn; Vn[:, :3, 3] = tn; Vn[:, 3, 3] = 1.0
    campos = -(Rn.transpose(1, 2) @ tn[:, :, None])[:, :, 0]
    return Vn.numpy(), campos.numpy(), m.numpy(), v.numpy(), delta.numpy()


def ulp_bound(ref, n_ulp=2):
    """n_ulp float32 ulps of the view's largest entry magnitude: [C]"""
    big = np.abs(np.asarray(ref, np.float64)).reshape(ref.shape[0], -1).max(1).astype(np.float32)
    return n_ulp * np.spacing(big).astype(np.float64)
