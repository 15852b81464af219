"""CPU pins of tests/project_cases.py -- the inputs of test_gpu_project.py -- with the C oracle and float64 torch alone (no
GPU): every case reaches the branch it names (its predicate is asserted, not assumed), the oracle's forward agrees with
gs_torch_ref.project in float64 on every visible pair, and the oracle's hand-written backward stays near float64 autograd
on asymmetric cameras, clamped pairs, culled pairs and every other planted edge.

What existed before: test_oracle_gs.test_backward_matches_fp64_autograd compares the oracle's backward with float64 on two
random scenes of st3r_synth.make_scene, whose cameras are symmetric (fx == fy, centred principal point) and clamp nothing,
end to end through the dense renderer, to 2e-3 of each tensor's maximum.  It stays as it is; test_backward_near_float64
below is the same figure on the chain rule alone, per GAUSSIAN (each against its own gradient), on the planted cases.
"""
import numpy as np
import pytest
import torch

import project_cases as pc
from oracle import gs_torch_ref as tr

ALL = list(pc.CASES)
U = pc.U


@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_branch(oracle_built, name):
    case = pc.get(name)
    O = pc.reference(name)["O"]
    case.check(case, O)
    # the layout every test relies on: a culled pair is twelve zero floats and no tile
    dead = ~O["vis"]
    assert not O["records"][dead].any() and not O["tiles"][dead].any()
    assert (O["radii"][O["vis"]] > 0).all() and not O["records"][:, 11].any()


def test_cameras_are_asymmetric_and_one_is_turned(oracle_built):
    for name in ALL:
        case = pc.get(name)
        for K in case.Ks:
            assert K[0, 0] != K[1, 1] and K[0, 2] != 0.5 * case.W and K[1, 2] != 0.5 * case.H, name
            L = pc.limits(K, case.W, case.H)
            assert L[0] != L[1] and L[2] != L[3], name
        R = case.viewmats[:, :3, :3]
        turned = (np.abs(R) > 0.02).sum((1, 2)) >= 8                 # no permutation: (nearly) every entry is non-zero
        moved = np.abs(case.campos()).max(1) > 0.1
        assert (turned & moved).any(), name


@pytest.mark.parametrize("name", ALL)
def test_forward_agrees_with_float64(oracle_built, name):
    """means2d, depth and conic of every visible pair.  The tolerances follow float32 rounding of the inputs' magnitudes:

      p = R m + t      three products, three additions: |error| <= 5 u S, S = sum_j |R_ij m_j| + |t_i| (gamma_4, rounded up)
      depth            = p_z: 5 u S_z
      means2d          fx x / z + cx: the errors of x and z carried through (fx (e_x / z + |x| e_z / z^2)), three more
                       roundings on fx x / z (product, reciprocal, product) and one on the sum: 4 u |fx x / z| + u |m2x|
      conic            cov2d = J Rc Rq diag(s^2) Rq^T Rc^T J^T + eps2d I runs through about 32 rounded stages (quaternion
                       norm 4, rotation 3, M 1, M M^T 3, R cov 3, . R^T 3, limits and J 6, J S 3, . J^T 3, + eps2d 1 ...),
                       each on sums whose absolute terms are bounded by A = 3 smax^2 Jn^2 (Jn = the larger absolute row
                       sum of J, 3 >= the squared absolute row sums of two rotations): E = 32 u (A + eps2d) per entry.
                       conic = adj(cov2d) / det: |error| <= E / det + |conic| e_det / det with e_det <= 2 E (c00 + c11)."""
    case = pc.get(name)
    O = pc.reference(name)["O"]
    vis = O["vis"].reshape(case.Cn, case.N)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    means, quats, scales = t(case.means), t(case.quats), t(case.scales)
    smax2 = float(np.abs(case.scales).max()) ** 2
    worst = dict(means2d=0.0, depth=0.0, conic=0.0)
    pcs = case.cam_coords()
    for c in range(case.Cn):
        idx = np.nonzero(vis[c])[0]
        if idx.size == 0:
            continue
        m2, z, conic = tr.project(means[idx], quats[idx], scales[idx], t(case.viewmats[c]), t(case.Ks[c]), case.W, case.H,
                                  case.kw["eps2d"])
        m2, z, conic = m2.numpy(), z.numpy(), conic.numpy()
        rec = O["records"][c * case.N + idx].astype(np.float64)
        R = np.abs(case.viewmats[c, :3, :3].astype(np.float64)); tt = np.abs(case.viewmats[c, :3, 3].astype(np.float64))
        S = np.abs(case.means[idx].astype(np.float64)) @ R.T + tt
        e = 5 * U * S
        p = pcs[c, idx]
        assert np.allclose(p[:, 2], z, rtol=1e-12)
        fx, fy = float(case.Ks[c, 0, 0]), float(case.Ks[c, 1, 1])
        tol_z = e[:, 2]
        tol_m = np.stack([
            fx * (e[:, 0] / z + np.abs(p[:, 0]) * e[:, 2] / z ** 2) + 4 * U * np.abs(fx * p[:, 0] / z) + U * np.abs(m2[:, 0]),
            fy * (e[:, 1] / z + np.abs(p[:, 1]) * e[:, 2] / z ** 2) + 4 * U * np.abs(fy * p[:, 1] / z) + U * np.abs(m2[:, 1])], 1)
        L = pc.limits(case.Ks[c], case.W, case.H)
        cj = fx * np.minimum(np.abs(p[:, 0] / z), max(L[0], L[1])) / z
        d = fy * np.minimum(np.abs(p[:, 1] / z), max(L[2], L[3])) / z
        Jn = np.maximum(fx / z + cj, fy / z + d)
        E = 32 * U * (3 * smax2 * Jn ** 2 + case.kw["eps2d"])
        detc = conic[:, 0] * conic[:, 2] - conic[:, 1] ** 2          # = 1 / det(cov2d)
        tr2 = (conic[:, 0] + conic[:, 2]) / detc                     # c00 + c11
        tol_c = E * detc * (1.0 + 2.0 * tr2 * np.abs(conic).max(1))
        for key, a, b, tol in (("means2d", rec[:, 0:2], m2, tol_m), ("depth", rec[:, 9], z, tol_z),
                               ("conic", rec[:, 3:6], conic, tol_c[:, None])):
            ratio = float((np.abs(a - b) / np.broadcast_to(tol, a.shape)).max())
            worst[key] = max(worst[key], ratio)
    print(name, "worst error / tolerance:", {k: "%.3f" % v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


SANITY = 2e-3       # test_oracle_gs.test_backward_matches_fp64_autograd's figure, here per Gaussian


@pytest.mark.parametrize("name", ALL)
def test_backward_near_float64(oracle_built, name):
    """The oracle's chain rule (float32 forward state, double sums) against float64 autograd, per Gaussian and parameter
    group: the yardstick of test_gpu_project.py.  Pins the oracle on asymmetric cameras and clamped pairs (a swap of two
    limits, or of fx and fy, in gso_project_sh_bwd moves the clamp cases' gradients by their own size).  The culled
    pairs' cotangents are NaN: none reaches either gradient."""
    R = pc.reference(name)
    case = pc.get(name)
    assert np.isnan(R["v"][~R["O"]["vis"]]).all() and np.isfinite(R["v"][R["O"]["vis"]]).all()
    pg = pc.per_gaussian(R["o32"], R["r64"])
    for k in pc.GROUPS:
        assert np.isfinite(R["o32"][k]).all() and np.isfinite(R["r64"][k]).all(), (name, k)
        err, scale = pg[k]
        b = R["bounds"][k]
        print("%s %s: oracle error %.1e of the Gaussian's own gradient -> bound %.1e" % (name, k, b["own"], b["rel"]))
        assert (err <= SANITY * scale).all(), (name, k, float((err / scale).max()))
    # a Gaussian visible nowhere: the regularisers' terms and nothing else
    nowhere = ~R["O"]["vis"].reshape(case.Cn, case.N).any(0)
    if nowhere.any():
        go_, gs_ = pc.reg_grads(case)
        for G in (R["o32"], R["r64"]):
            assert not G["means"][nowhere].any() and not G["quats"][nowhere].any() and not G["sh"][nowhere].any()
            assert np.array_equal(G["opacities"][nowhere], go_[nowhere]) and np.array_equal(G["scales"][nowhere], gs_[nowhere])
    assert float(np.abs(R["r64"]["means"]).max()) > 0


def test_sh_strides_are_the_same_case(oracle_built):
    a, b = pc.get("sh_stride_12"), pc.get("sh_stride_72")
    assert np.array_equal(a.sh, b.sh[:, :4]) and np.array_equal(a.means, b.means)
    A, B = pc.reference("sh_stride_12"), pc.reference("sh_stride_72")
    assert np.array_equal(A["O"]["records"].view(np.uint32), B["O"]["records"].view(np.uint32))
    for k in pc.GROUPS:
        assert np.array_equal(A["o32"][k], B["o32"][k]) and np.array_equal(A["r64"][k], B["r64"][k])


@pytest.mark.parametrize("which,slots", [("384", 384), ("385", 385), ("uneven", 399)])
def test_gather_scenes_slot_counts(oracle_built, which, slots):
    """the wave's slot count on both sides of 64 * GATHER_WIDE_ABOVE, with the reference rectangles and with the fused
    path's exact culling (blend_cases.tile_rects: tight == reference for every live pair), and every large pair's alpha
    passing 1/255 at a pixel centre of every tile (blend_cases.alpha_hit_counts, independent of every rectangle rule)"""
    import blend_cases as bc
    case = pc.gather_scene(which)
    O = pc.oracle_forward(case)
    tags = case.tags
    live = np.nonzero(O["vis"])[0].tolist()
    assert live == sorted(tags["big"] + tags["small"])
    assert int(O["tiles"].sum()) == slots
    assert all(int(O["tiles"][i]) == tags["tiles"] for i in tags["big"])
    assert all(int(O["tiles"][i]) == 1 for i in tags["small"])
    rec = O["records"]
    ref, tight = bc.tile_rects(rec[:, 0:2], O["radii"], rec[:, 2], rec[:, 3:6], -(-case.W // 16), -(-case.H // 16))
    assert np.array_equal(ref, tight)
    bcase = bc.Case(case.name, rec, 1, case.N, case.W, case.H)
    hits = bc.alpha_hit_counts(bcase)
    assert int(hits.sum()) == slots and int(hits.min()) == len(tags["big"])
    if which == "uneven":                       # one pair of >= 65 slots between empty pairs
        for i in tags["big"]:
            assert int(O["tiles"][i]) >= 65 and not O["tiles"][i - 1] and not O["tiles"][i + 1]
    # nothing saturates: eight opacities of 0.1
    assert 0.9 ** len(tags["big"]) * 0.5 > 0.2


def test_fused_shapes_are_visible(oracle_built):
    for N in pc.FUSED_N:
        case = pc.fused_shape(N)
        O = pc.oracle_forward(case)
        vis = O["vis"].reshape(2, N)
        assert vis[:, 0].any() and vis[:, N - 1].any() and int(O["tiles"].sum()) >= N
