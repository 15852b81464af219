"""Hand-built inputs for the dense point extraction (csrc/dense.hip): views of different sizes, planted rounding / depth /
confidence ties, and a case on which the order of the in-place update decides.  test_oracle_dense_cases.py pins every
case on oracle/dense_oracle.py alone; test_gpu_dense_cases.py runs them through `ops`.  Nothing is masked:

  * mixed sizes: general geometry; the inputs are nudged until the oracle's own decision margin (pixel rounding, depth
    test, z = 0) exceeds 2e-3 on EVERY point, so float32 and float64 take the same side everywhere;
  * planted / order / many-view cases: cameras with R = I and translations, focals, principal points, depths that are
    small dyadic numbers: projection, the rounding ties, 0.75 * depth are exact in binary32 and binary64 alike, so
    every confidence is compared for equal bits.
"""
import numpy as np

from oracle import dense_oracle as do

F = np.float32
CAM_STRIDE = 24


def cam_row(R, T, f, cx, cy, A=0.0, B=1.0):
    r = np.zeros(CAM_STRIDE, F)
    r[:9] = np.asarray(R, np.float64).reshape(-1); r[9:12] = T; r[12:17] = (f, cx, cy, A, B)
    return r


def oracle_cams(cam):
    """K and cam2w (float64) of the float32 camera rows -- exactly the numbers the kernel sees."""
    Ks, c2ws = [], []
    for r in np.asarray(cam, np.float64):
        Ks.append(np.array([[r[12], 0, r[13]], [0, r[12], r[14]], [0, 0, 1.0]]))
        m = np.eye(4); m[:3, :3] = r[:9].reshape(3, 3); m[:3, 3] = r[9:12]; c2ws.append(m)
    return Ks, c2ws


def split(a, sizes):
    start = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
    return [a[start[k]:start[k + 1]] for k in range(len(sizes))]


def view_start(sizes):
    return np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int32)


def clean_oracle(case, conf, pts, zcam, tol, bad_conf, margin=None, order=None):
    """oracle.clean_pointcloud on the concatenated arrays; `order`: a permutation of the views to evaluate in."""
    sizes = case["sizes"]
    Ks, c2ws = oracle_cams(case["cam"])
    cf, pt, zm = split(np.asarray(conf), sizes), split(np.asarray(pts, np.float64), sizes), split(np.asarray(zcam, np.float64), sizes)
    o = list(range(len(sizes))) if order is None else list(order)
    res = do.clean_pointcloud([cf[k] for k in o], [Ks[k] for k in o], [c2ws[k] for k in o], [zm[k] for k in o],
                              [pt[k] for k in o], [sizes[k] for k in o], tol=tol, bad_conf=bad_conf, margin=margin)
    out = [None] * len(sizes)
    for pos, k in enumerate(o):
        out[k] = res[pos]
    return np.concatenate(out)


def clean_vectorised(case, conf, pts, zcam, tol, bad_conf, snapshot=False):
    """The same function with the inner loop over j done at once (float64): view i's point ends at min(c, bad_conf) iff
    SOME j finds it in front and less confident -- once lowered it can only be found again, with the same result.
    `snapshot`: compare against the confidences as they were before any cleaning (what the kernel must NOT do)."""
    sizes = np.asarray(case["sizes"]); start = view_start(case["sizes"]).astype(np.int64)
    cam = np.asarray(case["cam"], np.float64)
    R = cam[:, :9].reshape(-1, 3, 3); T = cam[:, 9:12]; f = cam[:, 12]; cx = cam[:, 13]; cy = cam[:, 14]
    C = len(sizes)
    live = np.asarray(conf, np.float64).copy(); orig = live.copy()
    pts = np.asarray(pts, np.float64); zcam = np.asarray(zcam, np.float64)
    for i in range(C):
        p = pts[start[i]:start[i + 1]]
        d = p[None] - T[:, None]                                   # [C, n, 3]
        q = np.einsum("jab,jna->jnb", R, d)                        # R^T d
        z = q[..., 2]
        with np.errstate(all="ignore"):
            u = np.rint((f[:, None] * q[..., 0] + cx[:, None] * z) / z)
            v = np.rint((f[:, None] * q[..., 1] + cy[:, None] * z) / z)
        H, W = sizes[:, 0][:, None], sizes[:, 1][:, None]
        inside = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        inside[i] = False
        k = np.where(inside, start[:C, None] + v * W + u, 0).astype(np.int64)
        ci = live[start[i]:start[i + 1]]
        ref = orig if snapshot else live
        bad = inside & (z < (1 - tol) * zcam[k]) & (ci[None] < ref[k])
        low = bad.any(0)
        live[start[i]:start[i + 1]] = np.where(low, np.minimum(ci, bad_conf), ci)
    return live


# ------------------------------------------------------------------------------------------------- 1. mixed sizes
def look_at(eye):
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack([right, down, fwd], 1), eye


MIXED = {"c3": [(5, 7), (16, 16), (3, 40)], "c4": [(5, 7), (1, 1), (3, 40), (16, 16)], "c1": [(9, 11)]}


def mixed_case(name, G=23):
    """Every view with its own size, focal, principal point, A, B and base focal, so that a pixel unprojected with
    another view's row lands somewhere else.  Offsets are nudged (deterministically) until every point clears the
    oracle's decision margin of 2e-3."""
    sizes = MIXED[name]
    C = len(sizes)
    rng = np.random.default_rng(len(name) + 10 * C)
    cam = np.zeros((C, CAM_STRIDE), F)
    pix, idxs, offs, confs = [], [], [], []
    for k, (H, W) in enumerate(sizes):
        R, T = look_at(np.array([3 * np.cos(0.5 * k), 3 * np.sin(0.5 * k), 0.4 + 0.2 * k]))
        fk = 0.9 * max(W, H, 8) * (1 + 0.07 * k)
        cam[k] = cam_row(R, T, fk, W / 2 + 0.3 * k, H / 2 - 0.2 * k, rng.uniform(-0.1, 0.1), rng.uniform(2.0, 3.5))
        ys, xs = np.mgrid[0:H, 0:W]
        pix.append(np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], -1))
        idxs.append(rng.integers(0, G, H * W))
        o = 1 + 0.05 * np.sin(xs / 7 + k) * np.cos(ys / 5)
        o = o.reshape(-1)
        fl = rng.choice(H * W, max(1, H * W // 10), replace=False)
        o[fl] *= rng.uniform(0.5, 0.8, len(fl))
        offs.append(o)
        confs.append(rng.uniform(1.0, 4.0, H * W))
    case = dict(name=name, C=C, G=G, sizes=sizes, cam=cam, start=view_start(sizes),
                pix=np.concatenate(pix).astype(F), idx=np.concatenate(idxs).astype(np.int32),
                core=rng.uniform(0.8, 1.2, (C, G)).astype(F), base_f=(rng.uniform(0.8, 1.1, C) * cam[:, 12]).astype(F),
                conf=np.concatenate(confs).astype(F))
    off = np.concatenate(offs).astype(F)
    for it in range(40):
        case["off"] = off
        pts, z = unproject_ref(case)
        m = []
        clean_oracle(case, case["conf"], pts.astype(F), z.astype(F), 0.001, 0.0, margin=m)
        m = np.concatenate(m) if C > 1 else np.full(len(off), np.inf)
        tight = m <= 4e-3
        if not tight.any():
            break
        off = np.where(tight, off * F(1.0 + 0.004 * (it + 1)), off).astype(F)
    case["off"] = off
    return case


def unproject_ref(case):
    """float64 oracle on the float32 inputs, all views concatenated."""
    Ks, c2ws = oracle_cams(case["cam"])
    pts, zs = [], []
    pix, idx, off = (split(case[k], case["sizes"]) for k in ("pix", "idx", "off"))
    for k in range(case["C"]):
        r = case["cam"][k].astype(np.float64)
        dm = r[15] + r[16] * case["core"][k].astype(np.float64)
        a, b = do.unproject(pix[k].astype(np.float64), idx[k], off[k], dm, Ks[k], c2ws[k], case["base_f"][k])
        pts.append(a); zs.append(b)
    return np.concatenate(pts), np.concatenate(zs)


def many_views_case(C):
    """C views of 4 x 4 in a row (R = I, camera k at x = k, f = 4, principal point (2, 2)), every pixel at depth 4 or 2
    (cores 4 and 2, A = 0, B = 1, offset 1): a point of view i lands exactly on a pixel centre of its neighbours, the
    depth-2 points float in front of the depth-4 surfaces.  Everything is exact in binary32."""
    sizes = [(4, 4)] * C
    rng = np.random.default_rng(C)
    cam = np.stack([cam_row(np.eye(3), (float(k), 0, 0), 4.0, 2.0, 2.0) for k in range(C)])
    ys, xs = np.mgrid[0:4, 0:4]
    pix = np.tile(np.stack([xs.reshape(-1), ys.reshape(-1)], -1), (C, 1)).astype(F)      # integer pixel coordinates
    return dict(name="many%d" % C, C=C, G=2, sizes=sizes, cam=cam, start=view_start(sizes), pix=pix,
                idx=rng.integers(0, 2, 16 * C).astype(np.int32), core=np.tile(np.array([4.0, 2.0], F), (C, 1)),
                base_f=np.full(C, 4.0, F), off=np.ones(16 * C, F), conf=rng.integers(1, 9, 16 * C).astype(F))


# ------------------------------------------------------------------------------------------------- 2. planted decisions
def planted_case():
    """View 0 (1 x n, camera behind everything: nobody projects into it) carries the planted points; view 1 (H x W =
    5 x 6, at the origin) and view 2 (4 x 5, at x = 16) are the targets: f = 2, principal point (0.5, 0.5), surface depth
    4, confidence 5 where column + row is even and 1 where it is odd.  tol = 0.25: a point is in front below depth 3.
    A planted point has confidence 3 unless stated: it is lowered iff it lands on an even pixel."""
    T1, T2 = np.zeros(3), np.array([16.0, 0, 0])
    rows = []          # (world point, confidence, what)

    def at(T, u, v, z=1.0, c=3.0, what=""):
        # the world point that projects to exactly (u, v) at depth z in a target at T: x = (u - 0.5) z / 2
        rows.append((np.array([T[0] + (u - 0.5) * z / 2, T[1] + (v - 0.5) * z / 2, T[2] + z]), c, what))

    for T, (H, W), tag in ((T1, (5, 6), "t1"), (T2, (4, 5), "t2")):
        at(T, 2.5, 0, what=tag + " u=2.5 -> column 2 (even: lowered)")
        at(T, 3.5, 0, what=tag + " u=3.5 -> column 4 (even: lowered)")
        at(T, 2.5, 1, what=tag + " u=2.5, row 1 -> (2, 1) odd: kept")
        at(T, -0.5, 0, what=tag + " u=-0.5 -> -0: inside, column 0 (lowered)")
        at(T, W - 0.5, 0, what=tag + " u=W-0.5 -> %s" % ("W: outside (kept)" if W % 2 == 0 else "W-1: inside, even (lowered)"))
        at(T, 0, 2.5, what=tag + " v=2.5 -> row 2 (lowered)")
        at(T, 0, 3.5, what=tag + " v=3.5 -> row 4: %s" % ("inside (lowered)" if H > 4 else "outside (kept)"))
        at(T, 1, 2.5, what=tag + " v=2.5, column 1 -> odd: kept")
        at(T, 0, -0.5, what=tag + " v=-0.5 -> -0: inside, row 0 (lowered)")
        at(T, 0, H - 0.5, what=tag + " v=H-0.5 -> %s" % ("H: outside (kept)" if H % 2 == 0 else "H-1: inside, even (lowered)"))
        at(T, 0.5, 0.5, z=3.0, what=tag + " z == 0.75 depth: not in front (kept)")
        at(T, 0.5, 0.5, z=float(np.nextafter(F(3), F(0))), what=tag + " z one float below 0.75 depth (lowered)")
        at(T, 0.5, 0.5, z=2.0, c=5.0, what=tag + " confidence equal to the pixel's (kept)")
        at(T, 0.5, 0.5, z=2.0, c=float(np.nextafter(F(5), F(0))), what=tag + " confidence one float below (lowered)")
        at(T, 0.5, 0.5, z=2.0, c=0.25, what=tag + " confidence below bad_conf = 0.5 (kept at 0.25)")
        rows.append((np.array([T[0], T[1], T[2] + 0.0]), 3.0, tag + " z == 0 (kept)"))
        rows.append((np.array([T[0], T[1], T[2] - 1.0]), 3.0, tag + " z < 0 (kept)"))
    n0 = len(rows)
    sizes = [(1, n0), (5, 6), (4, 5)]
    cam = np.stack([cam_row(np.eye(3), (0, 0, 1024.0), 2.0, 0.5, 0.5), cam_row(np.eye(3), T1, 2.0, 0.5, 0.5),
                    cam_row(np.eye(3), T2, 2.0, 0.5, 0.5)])
    pts = [np.stack([r[0] for r in rows])]; conf = [np.array([r[1] for r in rows])]; zc = [np.ones(n0)]
    for T, (H, W) in ((T1, (5, 6)), (T2, (4, 5))):
        ys, xs = np.mgrid[0:H, 0:W]
        u, v = xs.reshape(-1), ys.reshape(-1)
        pts.append(np.stack([T[0] + (u - 0.5) * 2.0, T[1] + (v - 0.5) * 2.0, np.full(H * W, T[2] + 4.0)], -1))
        conf.append(np.where((u + v) % 2 == 0, 5.0, 1.0)); zc.append(np.full(H * W, 4.0))
    pts, conf, zc = np.concatenate(pts), np.concatenate(conf), np.concatenate(zc)
    assert (pts.astype(F) == pts).all() and (conf.astype(F) == conf).all()
    return dict(name="planted", C=3, sizes=sizes, cam=cam, start=view_start(sizes), pts=pts.astype(F), zcam=zc.astype(F),
                conf=conf.astype(F), what=[r[2] for r in rows], tol=0.25)


# ------------------------------------------------------------------------------------------------- 3. order
def order_case():
    """f = 2, principal point (0.5, 0.5), R = I; view 0 (1 x 3) at the origin, view 1 (1 x 2) at x = 1, view 2 (1 x 1)
    behind everything.  tol = 0.25, bad_conf = 0.5.
      P0 = pixel 2 of view 0, depth 2, confidence 3: lands on pixel 1 of view 1 (depth 4, confidence 5) -> lowered to 0.5;
      Q1 = pixel 0 of view 1, depth 1, confidence 2: lands on pixel 2 of view 0 (P0's, depth 2), in front of it.
    In the reference's order (i = 0 first) Q1 meets P0's LOWERED confidence: 2 < 0.5 is false, Q1 keeps 2.  Evaluated
    in reverse, or against a snapshot of the confidences, Q1 meets 3 and is lowered."""
    def pt(T, u, z):
        return [T + (u - 0.5) * z / 2, (0 - 0.5) * z / 2, z]
    sizes = [(1, 3), (1, 2), (1, 1)]
    cam = np.stack([cam_row(np.eye(3), (0, 0, 0), 2.0, 0.5, 0.5), cam_row(np.eye(3), (1.0, 0, 0), 2.0, 0.5, 0.5),
                    cam_row(np.eye(3), (0, 0, 1024.0), 2.0, 0.5, 0.5)])
    pts = np.array([pt(0, 0, 4.0), pt(0, 1, 4.0), pt(0, 2, 2.0), pt(1, 0, 1.0), pt(1, 1, 4.0), [0, 0, 1030.0]])
    zc = np.array([4.0, 4.0, 2.0, 1.0, 4.0, 6.0]); conf = np.array([1.0, 1.0, 3.0, 2.0, 5.0, 1.0])
    return dict(name="order", C=3, sizes=sizes, cam=cam, start=view_start(sizes), pts=pts.astype(F), zcam=zc.astype(F),
                conf=conf.astype(F), tol=0.25, bad_conf=0.5)
