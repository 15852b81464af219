"""Numpy restatement of the per-view kernels (TEST INFRASTRUCTURE ONLY; no GPU, no C oracle): the per-pair terms of the pose
and intrinsics gradients (gs_pose_bwd.hip, gs_intrinsics.hip, conic_chain of project_common.h), their finishers, the launch
arrangement of the streaming kernels (per_view.h) and the moments per_view_adam_delta must store.

pose_pair_terms / intrinsics_pair_terms are vectorised over the visible pairs, in the order of the flat pair index
c * N + g.  dtype = float32: every operation of the kernels in the order they are written, with numpy's plain rounding (no
FMA contraction is mimicked); dtype = float64: the same formulas in double, with campos = inverse(V)[:3, 3] in double
instead of the float32 camera positions the kernels are handed.
"""
import fractions

import numpy as np

SH_C0, SH_C1 = 0.2820947917738781, 0.48860251190292
POSE_VALS = 15          # v_R (9, row major), v_t (3), v_campos (3)


def visible_pairs(records, N):
    """(flat pair indices, camera, Gaussian) of the pairs whose radius word is a positive integer"""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 12)
    pid = np.nonzero(rec[:, 10].view(np.int32) > 0)[0]
    if N == 0:
        return pid, pid, pid
    return pid, pid // N, pid % N


class _Pairs:
    """what both kernels compute per visible pair before they part: x y z, R, T = R Sigma, the clamp sides and conic_chain"""

    def __init__(self, case, records, v_splats, dtype):
        dt = np.dtype(dtype).type
        f = lambda a: np.asarray(a, dtype)
        c_ = lambda x: dt(x)
        pid, cam, g = visible_pairs(records, case.N)
        self.pid, self.cam, self.g, self.dt = pid, cam, g, dt
        rec = f(np.asarray(records, np.float32).reshape(-1, 12)[pid])
        v = f(np.asarray(v_splats, np.float32).reshape(-1, 12)[pid])
        self.rec, self.v = rec, v
        V = f(case.viewmats)[cam]
        R = [[V[:, i, j] for j in range(3)] for i in range(3)]
        K = f(case.Ks)[cam]
        fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
        W, H = c_(case.W), c_(case.H)
        tan_fovx, tan_fovy = c_(0.5) * W / fx, c_(0.5) * H / fy
        lim_xp, lim_xn = (W - cx) / fx + c_(0.3) * tan_fovx, cx / fx + c_(0.3) * tan_fovx
        lim_yp, lim_yn = (H - cy) / fy + c_(0.3) * tan_fovy, cy / fy + c_(0.3) * tan_fovy
        m = f(case.means)[g]
        mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
        q = f(case.quats)[g]
        qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        sc = f(case.scales)[g]
        inv_norm = c_(1.0) / np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        qw, qx, qy, qz = qw * inv_norm, qx * inv_norm, qy * inv_norm, qz * inv_norm
        x2, y2, z2, xy, xz, yz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz
        wx, wy, wz = qw * qx, qw * qy, qw * qz
        one, two = c_(1.0), c_(2.0)
        Rq = [one - two * (y2 + z2), two * (xy - wz), two * (xz + wy),
              two * (xy + wz), one - two * (x2 + z2), two * (yz - wx),
              two * (xz - wy), two * (yz + wx), one - two * (x2 + y2)]
        M = [Rq[i * 3 + j] * sc[:, j] for i in range(3) for j in range(3)]
        cov = [M[0] * M[0] + M[1] * M[1] + M[2] * M[2], M[0] * M[3] + M[1] * M[4] + M[2] * M[5],
               M[0] * M[6] + M[1] * M[7] + M[2] * M[8], M[3] * M[3] + M[4] * M[4] + M[5] * M[5],
               M[3] * M[6] + M[4] * M[7] + M[5] * M[8], M[6] * M[6] + M[7] * M[7] + M[8] * M[8]]
        x = R[0][0] * mx + R[0][1] * my + R[0][2] * mz + V[:, 0, 3]
        y = R[1][0] * mx + R[1][1] * my + R[1][2] * mz + V[:, 1, 3]
        z = R[2][0] * mx + R[2][1] * my + R[2][2] * mz + V[:, 2, 3]
        T = [[None] * 3 for _ in range(3)]          # R Sigma
        for i in range(3):
            T[i][0] = R[i][0] * cov[0] + R[i][1] * cov[1] + R[i][2] * cov[2]
            T[i][1] = R[i][0] * cov[1] + R[i][1] * cov[3] + R[i][2] * cov[4]
            T[i][2] = R[i][0] * cov[2] + R[i][1] * cov[4] + R[i][2] * cov[5]
        Sxx = T[0][0] * R[0][0] + T[0][1] * R[0][1] + T[0][2] * R[0][2]
        Sxy = T[0][0] * R[1][0] + T[0][1] * R[1][1] + T[0][2] * R[1][2]
        Sxz = T[0][0] * R[2][0] + T[0][1] * R[2][1] + T[0][2] * R[2][2]
        Syy = T[1][0] * R[1][0] + T[1][1] * R[1][1] + T[1][2] * R[1][2]
        Syz = T[1][0] * R[2][0] + T[1][1] * R[2][1] + T[1][2] * R[2][2]
        Szz = T[2][0] * R[2][0] + T[2][1] * R[2][1] + T[2][2] * R[2][2]
        rz = one / z
        rz2 = rz * rz
        xr, yr = x * rz, y * rz
        self.x_in = (xr <= lim_xp) & (xr >= -lim_xn)
        self.y_in = (yr <= lim_yp) & (yr >= -lim_yn)
        tx = z * np.minimum(lim_xp, np.maximum(-lim_xn, xr))
        ty = z * np.minimum(lim_yp, np.maximum(-lim_yn, yr))
        a, cj, b, d = fx * rz, -fx * tx * rz2, fy * rz, -fy * ty * rz2
        # conic_chain.  The kernels take the conic from the pair's record (float32: the forward state); the double form
        # recomputes it, so that it is the operation itself and not the operation at a rounded conic
        A, B, Cc = rec[:, 3], rec[:, 4], rec[:, 5]
        if np.dtype(dtype) == np.float64:
            eps = c_(case.kw["eps2d"])
            c00 = a * a * Sxx + two * a * cj * Sxz + cj * cj * Szz + eps
            c01 = a * b * Sxy + a * d * Sxz + cj * b * Syz + cj * d * Szz
            c11 = b * b * Syy + two * b * d * Syz + d * d * Szz + eps
            det = c00 * c11 - c01 * c01
            A, B, Cc = c11 / det, -c01 / det, c00 / det
        vA, vB, vC = v[:, 3], c_(0.5) * v[:, 4], v[:, 5]
        X00, X01 = A * vA + B * vB, A * vB + B * vC
        X10, X11 = B * vA + Cc * vB, B * vB + Cc * vC
        G00 = -(X00 * A + X01 * B)
        G01 = -c_(0.5) * ((X00 * B + X01 * Cc) + (X10 * A + X11 * B))
        G11 = -(X10 * B + X11 * Cc)
        GJ00, GJ01, GJ02 = G00 * a, G01 * b, G00 * cj + G01 * d
        GJ10, GJ11, GJ12 = G01 * a, G11 * b, G01 * cj + G11 * d
        self.vS = dict(xx=a * GJ00, xy=a * GJ01, xz=a * GJ02, yy=b * GJ11, yz=b * GJ12, zz=cj * GJ02 + d * GJ12)
        self.vJ00 = two * (GJ00 * Sxx + GJ01 * Sxy + GJ02 * Sxz)
        self.vJ02 = two * (GJ00 * Sxz + GJ01 * Syz + GJ02 * Szz)
        self.vJ11 = two * (GJ10 * Sxy + GJ11 * Syy + GJ12 * Syz)
        self.vJ12 = two * (GJ10 * Sxz + GJ11 * Syz + GJ12 * Szz)
        self.fx, self.fy, self.x, self.y, self.z, self.rz, self.rz2, self.xr, self.yr = fx, fy, x, y, z, rz, rz2, xr, yr
        self.tx, self.ty, self.T, self.m = tx, ty, T, (mx, my, mz)


def pose_pair_terms(case, records, v_splats, dtype=np.float32, campos=None, info=None):
    """[pairs, 15]: what k_viewmat_bwd_part adds up per visible pair (v_R row major, v_t, v_campos).  campos: the camera
    positions the kernel is given (float32 mode; default case.campos()); float64 mode takes inverse(V)[:3, 3] in double.
    info: a dict that receives the branches taken per pair (x_in, y_in, colour_pass [pairs, 3]) and colour_margin, the
    smallest |colour before the clamp| of the pair"""
    P = _Pairs(case, records, v_splats, dtype)
    dt, rec, v = P.dt, P.rec, P.v
    out = np.zeros((P.pid.size, POSE_VALS), dtype)
    if P.pid.size == 0:
        return out
    if np.dtype(dtype) == np.float64:
        cp = np.linalg.inv(np.asarray(case.viewmats, np.float64))[:, :3, 3]
    else:
        cp = np.asarray(case.campos() if campos is None else campos, dtype)
    cp = np.asarray(cp, dtype)[P.cam]
    mx, my, mz = P.m
    k = np.asarray(case.sh, dtype).reshape(case.N, -1)[P.g, :12]
    c0, c1 = dt(SH_C0), dt(SH_C1)
    # SH backward: the gradient of the unnormalised direction d = m - campos
    dx, dy, dz = mx - cp[:, 0], my - cp[:, 1], mz - cp[:, 2]
    nrm = np.sqrt(dx * dx + dy * dy + dz * dz)
    inrm = dt(1.0) / nrm
    ux, uy, uz = dx * inrm, dy * inrm, dz * inrm
    vdx = vdy = vdz = np.zeros_like(ux)
    f64 = np.dtype(dtype) == np.float64
    margin = np.full(ux.shape, np.inf)
    passed = []
    for ch in range(3):
        pre = c0 * k[:, ch] + c1 * ((-uy * k[:, 3 + ch] + uz * k[:, 6 + ch]) - ux * k[:, 9 + ch]) + dt(0.5)
        passes = (pre >= 0) if f64 else ((rec[:, 6 + ch] > 0) | (pre >= 0))     # (the record's colour: float32 state)
        vc = np.where(passes, v[:, 6 + ch], dt(0.0))
        margin = np.minimum(margin, np.abs(pre))
        passed.append(passes)
        vdx = vdx + -c1 * k[:, 9 + ch] * vc
        vdy = vdy + -c1 * k[:, 3 + ch] * vc
        vdz = vdz + c1 * k[:, 6 + ch] * vc
    if info is not None:
        info.update(x_in=P.x_in, y_in=P.y_in, colour_pass=np.stack(passed, 1), colour_margin=margin)
    dotp = vdx * ux + vdy * uy + vdz * uz
    out[:, 12] = -((vdx - dotp * ux) * inrm)
    out[:, 13] = -((vdy - dotp * uy) * inrm)
    out[:, 14] = -((vdz - dotp * uz) * inrm)
    # projection backward
    fx, fy, x, y, rz, rz2 = P.fx, P.fy, P.x, P.y, P.rz, P.rz2
    rz3 = rz2 * rz
    vm2x, vm2y = v[:, 0], v[:, 1]
    two = dt(2.0)
    vpx = fx * rz * vm2x
    vpy = fy * rz * vm2y
    vpz = -(fx * x * vm2x + fy * y * vm2y) * rz2
    vpz = vpz + (-fx * rz2 * P.vJ00 - fy * rz2 * P.vJ11)
    vpx = np.where(P.x_in, vpx + -fx * rz2 * P.vJ02, vpx)
    vpz = np.where(P.x_in, vpz + two * fx * x * rz3 * P.vJ02, vpz + fx * P.tx * rz3 * P.vJ02)
    vpy = np.where(P.y_in, vpy + -fy * rz2 * P.vJ12, vpy)
    vpz = np.where(P.y_in, vpz + two * fy * y * rz3 * P.vJ12, vpz + fy * P.ty * rz3 * P.vJ12)
    S = P.vS
    vSm = [[S["xx"], S["xy"], S["xz"]], [S["xy"], S["yy"], S["yz"]], [S["xz"], S["yz"], S["zz"]]]
    vp, m, T = (vpx, vpy, vpz), P.m, P.T
    for i in range(3):
        for j in range(3):
            out[:, i * 3 + j] = vp[i] * m[j] + two * (vSm[i][0] * T[0][j] + vSm[i][1] * T[1][j] + vSm[i][2] * T[2][j])
        out[:, 9 + i] = vp[i]
    return out


def intrinsics_pair_terms(case, records, v_splats, dtype=np.float32):
    """[pairs, 4]: what k_intrinsics_bwd_part adds up per visible pair (v_fx, v_fy, v_cx, v_cy)"""
    P = _Pairs(case, records, v_splats, dtype)
    out = np.zeros((P.pid.size, 4), dtype)
    if P.pid.size == 0:
        return out
    vm2x, vm2y = P.v[:, 0], P.v[:, 1]
    v_fx = vm2x * P.xr + P.vJ00 * P.rz
    v_fy = vm2y * P.yr + P.vJ11 * P.rz
    out[:, 0] = np.where(P.x_in, v_fx + -P.x * P.rz2 * P.vJ02, v_fx)
    out[:, 1] = np.where(P.y_in, v_fy + -P.y * P.rz2 * P.vJ12, v_fy)
    out[:, 2] = np.where(P.x_in, vm2x, vm2x + P.vJ02 * P.rz)
    out[:, 3] = np.where(P.y_in, vm2y, vm2y + P.vJ12 * P.rz)
    return out


def camera_sums(terms, cam, Cn, absolute=False):
    """[Cn, NV] float64: the pairs' terms (or their absolute values) added per camera in double"""
    t = np.asarray(terms, np.float64)
    out = np.zeros((Cn, t.shape[1]))
    np.add.at(out, cam, np.abs(t) if absolute else t)
    return out


def pose_finish(sum15, V, absolute=False):
    """k_viewmat_bwd_finish in double: v_V = [[v_R, v_t], [0, 0]] - (V^-T [v_campos; 0]) (x) inverse(V)[:, 3] for one
    camera; absolute: the same with absolute values throughout and a plus sign (the entry scale)"""
    s = np.asarray(sum15, np.float64)
    inv = np.linalg.inv(np.asarray(V, np.float64))
    base = np.zeros((4, 4))
    base[:3, :3] = s[0:9].reshape(3, 3); base[:3, 3] = s[9:12]
    if absolute:
        u = np.abs(inv[:3, :]).T @ np.abs(s[12:15])
        return np.abs(base) + np.outer(u, np.abs(inv[:, 3]))
    u = inv[:3, :].T @ s[12:15]
    return base - np.outer(u, inv[:, 3])


def intrinsics_finish(sum4):
    """k_stream_finish<4>: a plain sum, nothing after it"""
    return np.asarray(sum4, np.float64)


# ---- the streaming kernels' launch arrangement (per_view.h) ----
STREAM_T = 256
STREAM_ALIGN = 1024
STREAM_MAX_WG = 256 * 8


def stream_grid(C, HW):
    """(workgroups per view, pixels per workgroup, want): stream_grid of per_view.h; want is the uncapped ceil(C HW / 1024)"""
    want_raw = (C * HW + STREAM_ALIGN - 1) // STREAM_ALIGN
    want = min(want_raw, STREAM_MAX_WG)
    b = max(want // C, 1)
    ch = (HW + b - 1) // b
    ch = (ch + STREAM_ALIGN - 1) // STREAM_ALIGN * STREAM_ALIGN
    return (HW + ch - 1) // ch, ch, want_raw


def vec(HW, aligned):
    """the 16-byte kernel runs: HW a multiple of 4 and every buffer on a 16-byte boundary"""
    return HW % 4 == 0 and bool(aligned)


def trips(pixels, is_vec):
    """trips of a thread's stride loop over a workgroup of `pixels` pixels (the busiest thread's)"""
    per = STREAM_T * (4 if is_vec else 1)
    return (pixels + per - 1) // per


def stream_tags(C, HW, aligned=True):
    """what a shape reaches, from the formulas alone"""
    blocks, chunk, want = stream_grid(C, HW)
    v = vec(HW, aligned)
    last = HW - (blocks - 1) * chunk
    per_thread = 4 if v else 1
    return dict(vec=v, blocks=blocks, chunk=chunk, trips=trips(min(chunk, HW), v), last=last,
                last_trips=trips(last, v), last_live_threads=-(-(last - (trips(last, v) - 1) * STREAM_T * per_thread) // per_thread),
                short_last=last < chunk, wraps=blocks > STREAM_T, want_zero=want // C == 0, cap=want > STREAM_MAX_WG,
                odd_base=C > 1 and (HW % 4) != 0)


# ---- per-view Adam ----
def adam_moments_exact(m, v, g, b1, b2, m_last, doubles=False):
    """the float32 moments per_view_adam_delta<m_last> must store, from float32 m, v and the double gradient g (arrays of
    one shape).  The rounded products are formed in double as the function spells them; the fused sum is exact rational
    arithmetic converted to the nearest double (Fraction -> float is correctly rounded: the hardware fma), then cast to
    float32.  doubles: also the two doubles before the cast (the step is formed from them)."""
    m64, v64, g64 = (np.asarray(a, np.float64) for a in (np.asarray(m, np.float32), np.asarray(v, np.float32), g))
    F = fractions.Fraction
    w1 = 1.0 - b1
    mi64, vi64 = np.empty(m64.shape), np.empty(m64.shape)
    for i in np.ndindex(m64.shape):
        mi, vi, gi = float(m64[i]), float(v64[i]), float(g64[i])
        if not (np.isfinite(mi) and np.isfinite(vi) and np.isfinite(gi)):
            raise ValueError("adam_moments_exact: finite inputs only")
        if m_last:      # fma(b1, m, w1 * g)
            mi64[i] = float(F(b1) * F(mi) + F(w1 * gi))
        else:           # fma(w1, g, b1 * m)
            mi64[i] = float(F(w1) * F(gi) + F(b1 * mi))
        vi64[i] = float(F((1.0 - b2) * gi) * F(gi) + F(b2 * vi))      # fma((1 - b2) g, g, b2 v)
    mo, vo = mi64.astype(np.float32), vi64.astype(np.float32)
    return (mo, vo, mi64, vi64) if doubles else (mo, vo)


def adam_delta(m_new, v_new, lr, b1, b2, eps, step):
    """-lr mhat / (sqrt(vhat) + eps) from the DOUBLE moments (the kernels keep mi, vi in double for the step)"""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return -lr * (np.asarray(m_new, np.float64) / bc1) / (np.sqrt(np.asarray(v_new, np.float64) / bc2) + eps)
