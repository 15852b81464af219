"""Planted-edge parity of the per-view kernels -- everything behind per_view.h -- through the C ABI, on the hand-built
inputs of per_view_kernel_cases.py (test_oracle_per_view_cases.py shows on the CPU that every case reaches its edge):

a. k_viewmat_bwd_part / k_viewmat_bwd_finish (gs_pose_bwd.hip) and k_intrinsics_bwd_part (gs_intrinsics.hip) +
   k_stream_finish<4> on every case of project_cases.CASES and on n0, trip2, similarity_V, general_row3, cancel and
   dead_camera: every entry of v_viewmats (row 3 too) and v_Ks within ITS OWN bound of float64 autograd --
   4 max(own32 of the case, median own32) x S, S the sum of the entry's absolute float64 contributions -- NaN in every culled
   record and cotangent, the same bits from two calls, exact +0.0 where nothing contributes.
b. k_exposure_fwd / k_exposure_bwd<false | true>, k_dprior_loss<false | true>, k_weight_sums<., false | true> and
   k_stream_finish<1 | 2 | 12> on the stream shapes, each aligned and 4 bytes off a 16-byte boundary, on dyadic inputs:
   every per-pixel output and every sum compared with ==.
c. k_exposure_adam, k_intrinsics_adam, k_pose_adam: C = 1, 63, 64, 65, three beta pairs, steps 1, 2, 100000, masks
   1 / 0 / -0.0 / 1e-30; the stored moments of per_view_adam_delta<false> bit for bit (oracle.per_view_oracle.
   adam_moments_exact), the pose and tied-focal steps under the bars of test_pose_adam_kernel_vs_fp64.

Measured on MI355X: MEASURED at the end of this file.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import per_view_kernel_cases as kc
from oracle import per_view_oracle as pvo

ALL = kc.PAIR_CASES
KINDS = ("pose", "intrinsics")


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a device error ends the run: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error: %s" % e, returncode=3)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def dev_at(a, off):
    """a float32 copy of `a` on the device that starts `off` floats behind a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


def nan_at(shape, off):
    return dev_at(np.full(shape, np.nan, np.float32), off)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# a. pair cases
def run_pair_kernels(ctx, case, records, v, cams=None):
    """(v_viewmats [Cn,4,4], v_Ks [Cn,4]) as float32 numpy; outputs preset to NaN.  N = 0 goes through the C ABI directly:
    an empty tensor has no address and ops would hand the library a NULL."""
    from starst3r_amd import ops, _lib
    N = case.N
    cams = list(range(case.Cn)) if cams is None else cams
    Cn = len(cams)
    vm, K, campos = dev(case.viewmats[cams]), dev(case.Ks[cams]), dev(case.campos()[cams])
    out_v = torch.full((Cn, 4, 4), float("nan"), device="cuda:0"); out_k = torch.full((Cn, 4), float("nan"), device="cuda:0")
    if N == 0:
        d = torch.zeros(16, device="cuda:0")
        p, lib = ops._p, _lib.lib()
        _lib.check(lib.st3r_gs_viewmat_bwd(ctx.handle, ops._stream(), 0, Cn, p(d), p(d), p(d), p(d), 12, p(vm), p(K), p(campos),
                                           case.W, case.H, case.kw["eps2d"], p(d), p(d), p(out_v)))
        _lib.check(lib.st3r_gs_intrinsics_bwd(ctx.handle, ops._stream(), 0, Cn, p(d), p(d), p(d), p(vm), p(K), case.W, case.H,
                                              case.kw["eps2d"], p(d), p(d), p(out_k)))
    else:
        rows = np.concatenate([np.arange(c * N, (c + 1) * N) for c in cams])
        means, quats, scales, sh = dev(case.means), dev(case.quats), dev(case.scales), dev(case.sh)
        splats, vs = dev(records[rows]), dev(v[rows])
        ops.viewmat_bwd(ctx, means, quats, scales, sh, vm, K, campos, case.W, case.H, splats, vs, eps2d=case.kw["eps2d"],
                        out=out_v)
        ops.intrinsics_bwd(ctx, means, quats, scales, vm, K, case.W, case.H, splats, vs, eps2d=case.kw["eps2d"], out=out_k)
    torch.cuda.synchronize()
    return host(out_v), host(out_k)


@pytest.mark.parametrize("name", ALL)
def test_pair_kernels_vs_float64(ctx, name):
    R = kc.pair_reference(name)
    case = R["case"]
    got = dict(zip(KINDS, run_pair_kernels(ctx, case, R["records"], R["v"])))
    again = dict(zip(KINDS, run_pair_kernels(ctx, case, R["records"], R["v"])))
    for kind in KINDS:
        G, K, rel = got[kind], R[kind], kc.rel_bounds(kind)[name]
        assert np.array_equal(G.view(np.uint32), again[kind].view(np.uint32)), (name, kind)          # no atomics
        assert np.isfinite(G).all(), "a culled pair's NaN (record or cotangent) or an unwritten entry leaked"
        S, err = K["S"], np.abs(G.astype(np.float64) - K["r64"])
        worst = float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
        print("%s %s: worst entry error %.2e of its scale = %.3f of the bound %.1e (the float32 oracle's own %.1e)"
              % (name, kind, worst, worst / rel, rel, K["own32"]))
        assert (err <= rel * S).all(), (name, kind, worst, rel, np.argwhere(err > rel * S)[:4].tolist())
        # nothing contributes: +0.0 on every bit (all of n0, dead_camera's middle camera, row 3 of a camera at the origin)
        assert not G.view(np.uint32)[S == 0].any(), (name, kind)
    if name == "n0":
        assert not got["pose"].view(np.uint32).any() and not got["intrinsics"].view(np.uint32).any()
        assert got["pose"].shape == (2, 4, 4) and got["intrinsics"].shape == (2, 4)
    if name == "dead_camera":
        assert not got["pose"][1].view(np.uint32).any() and not got["intrinsics"][1].view(np.uint32).any()
        sub = dict(zip(KINDS, run_pair_kernels(ctx, case, R["records"], R["v"], cams=[0, 2])))
        for kind in KINDS:                       # the neighbours: the bits they have without the dead camera between them
            assert np.array_equal(sub[kind].view(np.uint32), got[kind][[0, 2]].view(np.uint32)), kind
    if name == "views_c256":
        assert case.Cn == 256 and got["pose"].shape == (256, 4, 4)


def test_sh_strides_give_the_same_bits(ctx):
    a, b = kc.pair_reference("sh_stride_12"), kc.pair_reference("sh_stride_72")
    assert a["case"].sh.shape[1:] == (4, 3) and b["case"].sh.shape[1:] == (24, 3) and np.isnan(b["case"].sh[:, 4:]).all()
    ga, _ = run_pair_kernels(ctx, a["case"], a["records"], a["v"])
    gb, _ = run_pair_kernels(ctx, b["case"], b["records"], b["v"])
    assert np.isfinite(ga).all() and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# b. stream cases
OFFSETS = (0, 1)        # floats behind a 16-byte boundary: aligned, and 4 bytes off


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", kc.EXPOSURE_SHAPES)
def test_exposure_stream_is_exact(ctx, shape, off):
    from starst3r_amd import ops
    C, H, W = shape
    x, vy, E = kc.exposure_inputs(shape)
    y64, vx64, vE64 = kc.exposure_reference(x, vy, E)
    tags = kc.shape_tags(shape, aligned=off == 0)
    assert tags["vec"] == (off == 0 and (H * W) % 4 == 0)
    xd, vyd, Ed = dev_at(x, off), dev_at(vy, off), dev(E)
    y = ops.exposure_fwd(ctx, xd, Ed, out=nan_at(x.shape, off))
    vx, vE = ops.exposure_bwd(ctx, xd, Ed, vyd, v_rgb=nan_at(x.shape, off), v_exposure=torch.full((C, 3, 4), float("nan"), device="cuda:0"))
    alias = dev_at(vy, off)
    vx2, vE2 = ops.exposure_bwd(ctx, xd, Ed, alias, v_rgb=alias)                         # in place
    torch.cuda.synchronize()
    assert np.array_equal(host(y).astype(np.float64), y64)
    assert np.array_equal(host(vx).astype(np.float64), vx64) and np.array_equal(host(vx2).astype(np.float64), vx64)
    want = vE64.astype(np.float32)                                   # the float32 rounding of an exact sum
    assert np.array_equal(host(vE), want) and np.array_equal(host(vE2), want)
    assert np.array_equal(host(xd), x) and np.array_equal(host(vyd), vy)                # the inputs are left alone


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", kc.STREAM_SHAPES)
def test_depth_prior_and_weight_sums_are_exact(ctx, shape, off):
    from starst3r_amd import ops
    C, H, W = shape
    D, alpha, Z, w, tie = kc.depth_inputs(shape)
    ref = kc.depth_reference(D, alpha, Z, w)
    tags = kc.shape_tags(shape, aligned=off == 0)
    assert tags["vec"] == (off == 0 and (H * W) % 4 == 0)
    Dd, ad = dev_at(D[..., None], off), dev_at(alpha[..., None], off)
    Zd, wd = dev_at(Z, off), dev_at(w, off)
    sums, v_d, v_a = ops.loss_depth_prior(ctx, Dd, ad, Zd, wd, kc.DEPTH_FAC)
    torch.cuda.synchronize()
    s = host(sums)
    assert s.dtype == np.float64
    assert np.array_equal(s[:, 1], ref["n_c"]), (s[:, 1] - ref["n_c"])                  # k_weight_sums<., false>, finish<1>
    assert np.array_equal(s[:, 0], ref["sums"]), (s[:, 0] - ref["sums"])                # k_dprior_loss, finish<1>
    vd, va = host(v_d)[..., 0].astype(np.float64), host(v_a)[..., 0].astype(np.float64)
    assert np.array_equal(vd, ref["v_depth"]), int((vd != ref["v_depth"]).sum())
    assert np.array_equal(va, ref["v_alpha"]), int((va != ref["v_alpha"]).sum())
    off_w = ~(w > 0)                                                 # w <= 0 or NaN: exactly 0, whatever Z holds (NaN, inf)
    assert not vd[off_w].any() and not va[off_w].any()
    assert not va[alpha < kc.DP_MIN_ALPHA].any()
    # the weighted image loss' normalisers: k_weight_sums<., true> and finish<2>
    n1, n2, _ = kc.weight_sums_reference(w)
    img = torch.zeros((C, H, W, 3), device="cuda:0")
    lsums, _ = ops.loss_l1_ssim_weighted(ctx, img, img, wd, 0.8, 0.2, want_grad=False)
    torch.cuda.synchronize()
    ls = host(lsums)
    assert np.array_equal(ls[:, 2], n1) and np.array_equal(ls[:, 3], n2), (ls[:, 2:] - np.stack([n1, n2], 1))


# ---------------------------------------------------------------------------------------------------------------------
# c. Adam cases
LR = 1e-2


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _frozen_keeps_bits(A, before, after):
    fz = A["frozen"]
    for b, a in zip(before, after):
        assert np.array_equal(bits(a)[fz], b[fz])


@pytest.mark.parametrize("C", kc.ADAM_C)
def test_exposure_adam_moments_bit_for_bit(ctx, C):
    from starst3r_amd import ops
    for betas in kc.ADAM_BETAS:
        for step in kc.ADAM_STEPS:
            A = kc.adam_case("exposure", C, betas, step)
            E, G, m, v, mask = dev(A["param"]), dev(A["grad"]), dev(A["m"].reshape(-1)), dev(A["v"].reshape(-1)), dev(A["mask"])
            before = [bits(t).reshape(C, -1) for t in (E, m, v)]
            ops.exposure_adam_step(ctx, E, G, m, v, LR, betas[0], betas[1], kc.ADAM_EPS, step, mask)
            torch.cuda.synchronize()
            mo, vo, mi, vi = pvo.adam_moments_exact(A["m"], A["v"], A["grad"].reshape(C, 12).astype(np.float64), *betas, False,
                                                   doubles=True)
            live = ~A["frozen"]
            gm, gv, gE = host(m).reshape(C, 12), host(v).reshape(C, 12), host(E).reshape(C, 12)
            assert np.array_equal(gm.view(np.uint32)[live], mo.view(np.uint32)[live]), (C, betas, step)
            assert np.array_equal(gv.view(np.uint32)[live], vo.view(np.uint32)[live]), (C, betas, step)
            want = A["param"].reshape(C, 12).astype(np.float64) + pvo.adam_delta(mi, vi, LR, *betas, kc.ADAM_EPS, step)
            assert np.isfinite(gE).all()
            assert (np.abs(gE.astype(np.float64) - want)[live] <= _ulp32(want)[live]).all(), (C, betas, step)
            _frozen_keeps_bits(A, before, [t.reshape(C, -1) for t in (E, m, v)])
            if A["zero"] is not None:                                # zero gradient, zero moments: nothing moves, nothing is NaN
                z = A["zero"]
                assert np.array_equal(gE[z].view(np.uint32), A["param"].reshape(C, 12)[z].view(np.uint32))
                assert not gm[z].any() and not gv[z].any()


@pytest.mark.parametrize("C", kc.ADAM_C)
def test_intrinsics_adam_moments_bit_for_bit(ctx, C):
    """untied focals and the principal point: the gradient (fx v_fx, fy v_fy, W v_cx, H v_cy) is a product of two float32
    numbers in double, or a float32 times a power of two: exact, so the moments are those of adam_moments_exact"""
    from starst3r_amd import ops
    W, H = kc.ADAM_W, kc.ADAM_H
    for betas in kc.ADAM_BETAS:
        for step in kc.ADAM_STEPS:
            A = kc.adam_case("intrinsics", C, betas, step)
            K, G, m, v, mask = dev(A["param"]), dev(A["grad"]), dev(A["m"].reshape(-1)), dev(A["v"].reshape(-1)), dev(A["mask"])
            before = [bits(t).reshape(C, -1) for t in (K, m, v)]
            ops.intrinsics_adam_step(ctx, K, G, m, v, LR, betas[0], betas[1], kc.ADAM_EPS, step, mask, W, H, tie_focal=False,
                                     opt_pp=True)
            torch.cuda.synchronize()
            K0 = A["param"].astype(np.float64)
            q0 = np.stack([K0[:, 0, 0], K0[:, 1, 1], K0[:, 0, 2], K0[:, 1, 2]], 1)
            g = A["grad"].astype(np.float64) * np.array([1.0, 1.0, W, H])
            g[:, 0] *= q0[:, 0]; g[:, 1] *= q0[:, 1]
            mo, vo, mi, vi = pvo.adam_moments_exact(A["m"], A["v"], g, *betas, False, doubles=True)
            live = ~A["frozen"]
            gm, gv, gK = host(m).reshape(C, 4), host(v).reshape(C, 4), host(K)
            assert np.array_equal(gm.view(np.uint32)[live], mo.view(np.uint32)[live]), (C, betas, step)
            assert np.array_equal(gv.view(np.uint32)[live], vo.view(np.uint32)[live]), (C, betas, step)
            d = pvo.adam_delta(mi, vi, LR, *betas, kc.ADAM_EPS, step)
            want = np.stack([q0[:, 0] * np.exp(d[:, 0]), q0[:, 1] * np.exp(d[:, 1]), q0[:, 2] + W * d[:, 2], q0[:, 3] + H * d[:, 3]], 1)
            gq = np.stack([gK[:, 0, 0], gK[:, 1, 1], gK[:, 0, 2], gK[:, 1, 2]], 1).astype(np.float64)
            assert np.isfinite(gK).all() and (np.abs(gq - want)[live] <= _ulp32(want)[live]).all(), (C, betas, step)
            rest = np.ones((3, 3), bool); rest[0, 0] = rest[1, 1] = rest[0, 2] = rest[1, 2] = False
            assert np.array_equal(gK[:, rest].view(np.uint32), A["param"][:, rest].view(np.uint32))       # skew and row 2
            _frozen_keeps_bits(A, before, [t.reshape(C, -1) for t in (K, m, v)])
            if A["zero"] is not None:
                z = A["zero"]
                assert np.array_equal(gK[z].view(np.uint32), A["param"][z].view(np.uint32)) and not gm[z].any() and not gv[z].any()


@pytest.mark.parametrize("C", kc.ADAM_C)
def test_intrinsics_adam_tied_focal(ctx, C):
    """one focal scalar per view: its gradient fx v_fx + fy v_fy is a contracted double expression, so the bars are those of
    test_pose_adam_kernel_vs_fp64 (moments 1e-6 relative, parameters 2 float32 ulps of the view's largest entry); moment slot
    1 and, without opt_pp, the principal point and its moments keep every bit"""
    from starst3r_amd import ops
    W, H = kc.ADAM_W, kc.ADAM_H
    for betas in kc.ADAM_BETAS:
        for step in kc.ADAM_STEPS:
            A = kc.adam_case("intrinsics", C, betas, step)
            K, G, m, v, mask = dev(A["param"]), dev(A["grad"]), dev(A["m"].reshape(-1)), dev(A["v"].reshape(-1)), dev(A["mask"])
            before = [bits(t).reshape(C, -1) for t in (K, m, v)]
            ops.intrinsics_adam_step(ctx, K, G, m, v, LR, betas[0], betas[1], kc.ADAM_EPS, step, mask, W, H, tie_focal=True,
                                     opt_pp=False)
            torch.cuda.synchronize()
            K0, g4 = A["param"].astype(np.float64), A["grad"].astype(np.float64)
            g = K0[:, 0, 0] * g4[:, 0] + K0[:, 1, 1] * g4[:, 1]
            b1, b2 = betas
            rm = b1 * A["m"][:, 0].astype(np.float64) + (1 - b1) * g
            rv = b2 * A["v"][:, 0].astype(np.float64) + (1 - b2) * g * g
            e = np.exp(pvo.adam_delta(rm, rv, LR, b1, b2, kc.ADAM_EPS, step))
            live = ~A["frozen"]
            gm, gv, gK = host(m).reshape(C, 4), host(v).reshape(C, 4), host(K)
            for got, ref in ((gm[:, 0], rm), (gv[:, 0], rv)):
                rel = np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)
                assert (rel[live] <= 1e-6).all(), (C, betas, step, float(rel[live].max()))
            bound = kc.ulp_bound(K0)
            for i in (0, 1):
                assert (np.abs(gK[:, i, i].astype(np.float64) - K0[:, i, i] * e)[live] <= bound[live]).all(), (C, betas, step)
            keep = np.ones((3, 3), bool); keep[0, 0] = keep[1, 1] = False
            assert np.array_equal(gK[:, keep].view(np.uint32), A["param"][:, keep].view(np.uint32))
            assert np.array_equal(gm[:, 1:].view(np.uint32), A["m"][:, 1:].view(np.uint32))
            assert np.array_equal(gv[:, 1:].view(np.uint32), A["v"][:, 1:].view(np.uint32))
            _frozen_keeps_bits(A, before, [t.reshape(C, -1) for t in (K, m, v)])
            if A["zero"] is not None:
                z = A["zero"]
                assert np.array_equal(gK[z].view(np.uint32), A["param"][z].view(np.uint32)) and not gm[z, 0] and not gv[z, 0]


def _pose_step(ctx, A, lr):
    """one k_pose_adam step on the case against ref_pose_step: asserts the bars of test_pose_adam_kernel_vs_fp64 on the live
    views, every bit on the frozen ones; -> (V' float64 of the kernel, delta of the reference)"""
    from starst3r_amd import ops
    C, (b1, b2), step = A["C"], A["betas"], A["step"]
    V0 = A["param"]
    campos0 = (-(np.transpose(V0[:, :3, :3].astype(np.float64), (0, 2, 1)) @ V0[:, :3, 3:4].astype(np.float64))[:, :, 0]).astype(np.float32)
    V, cp, G, m, v, mask = dev(V0), dev(campos0), dev(A["grad"]), dev(A["m"].reshape(-1)), dev(A["v"].reshape(-1)), dev(A["mask"])
    before = [bits(t).reshape(C, -1) for t in (V, cp, m, v)]
    ops.pose_adam_step(ctx, V, cp, G, m, v, lr, b1, b2, kc.ADAM_EPS, step, mask)
    torch.cuda.synchronize()
    rV, rc, rm, rv, delta = kc.ref_pose_step(V0, A["grad"], A["m"], A["v"], lr, b1, b2, kc.ADAM_EPS, step)
    live = ~A["frozen"]
    gV, gc, gm, gv = host(V), host(cp), host(m).reshape(C, 6), host(v).reshape(C, 6)
    assert np.isfinite(gV).all() and np.isfinite(gc).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    for got, ref in ((gm, rm), (gv, rv)):
        rel = np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)
        assert (rel[live] <= 1e-6).all(), (C, A["betas"], step, lr, float(rel[live].max()))
    dV = np.abs(gV.astype(np.float64) - rV).reshape(C, -1).max(1)
    dc = np.abs(gc.astype(np.float64) - rc).max(1)
    assert (dV[live] <= kc.ulp_bound(rV)[live]).all(), (C, A["betas"], step, lr, float((dV / kc.ulp_bound(rV, 1))[live].max()))
    assert (dc[live] <= kc.ulp_bound(rc)[live]).all(), (C, A["betas"], step, lr, float((dc / kc.ulp_bound(rc, 1))[live].max()))
    R = gV[live, :3, :3].astype(np.float64)
    assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() <= 1e-6
    assert np.array_equal(gV[live, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (int(live.sum()), 1)))
    _frozen_keeps_bits(A, before, [t.reshape(C, -1) for t in (V, cp, m, v)])
    if A["zero"] is not None:        # the th2 < 1e-16 branch at delta = 0: without it 0 / 0
        z = A["zero"]
        assert not delta[z].any() and not gm[z].any() and not gv[z].any()
        assert np.array_equal(gV[z, :3, 3], V0[z, :3, 3]) and np.abs(gV[z].astype(np.float64) - V0[z]).max() <= 2 * 2.0 ** -24
    return gV.astype(np.float64), delta


@pytest.mark.parametrize("C", kc.ADAM_C)
def test_pose_adam_edges(ctx, C):
    for betas in kc.ADAM_BETAS:
        for step in kc.ADAM_STEPS:
            _pose_step(ctx, kc.adam_case("pose", C, betas, step), LR)


@pytest.mark.parametrize("lr", [1.0, 1.8, 1e-9])
def test_pose_adam_large_and_tiny_rotations(ctx, lr):
    """step 1 from zero moments: every |delta_i| = lr, a rotation by sqrt(3) lr -- 1.73 rad, 3.12 rad (near pi) and, at
    lr = 1e-9, the small-angle branch with a non-zero delta -- against matrix_exp in float64"""
    A = kc.adam_case("pose", 9, (0.9, 0.999), 1, zero_moments=True)
    gV, delta = _pose_step(ctx, A, lr)
    live = ~A["frozen"]; live[A["zero"]] = False
    assert live.sum() >= 4
    th = np.linalg.norm(delta[live, :3], axis=1)
    assert np.allclose(th, np.sqrt(3.0) * lr, rtol=1e-6)
    if lr == 1e-9:
        assert (th * th < 1e-16).all() and (th > 0).all()
        moved = np.abs(gV[live, :3, 3] - A["param"][live, :3, 3].astype(np.float64)).max()
        assert moved == 0.0 or moved <= 2.0 ** -22                   # (1e-9 is below half a float32 unit of t: V keeps its bits or so)


# MEASURED (MI355X):
#   pair kernels   all 35 cases within their bounds; worst kernel error / bound 0.42 (near_far, intrinsics), pose 0.37 (trip2);
#                  the bounds are 2.6e-7 .. 3.4e-6 (pose) and 1.2e-7 .. 7.1e-7 (intrinsics) of an entry's own scale S; the same
#                  bits from two calls; +0.0 wherever S = 0; dead_camera's neighbours keep the bits of the two-camera call
#   streams        every output and sum equal (==) on all 8 shapes x 2 alignments
#   Adam           exposure / untied intrinsics moments bit for bit on all 36 (C, betas, step) combinations each
# Run time: 85 cases, 5.3 s in pytest; the slowest 2.3 s (the first pair case computes the references of all 35, whose median
# the bounds need), every other below 0.2 s.
# Mutations (by hand, each run once; all four fail here): DESIGN.md, "Per-view kernels on every pair, sum, stream and Adam edge".
