"""CPU pins of tests/per_view_kernel_cases.py -- the inputs of test_gpu_per_view_cases.py -- with numpy, the C oracle's
forward and float64 torch alone (no GPU): every case reaches the edge it names, the numpy oracle of
oracle/per_view_oracle.py is the operation (float64 autograd through campos = inverse(V)[:3, 3]), the per-entry bounds
come from the float32 oracle's own error, the host formulas are those of per_view.h, the dyadic stream inputs add up
exactly in any order, and adam_moments_exact is Adam."""
import math
import os
import re

import numpy as np
import pytest

import per_view_kernel_cases as kc
import project_cases as pc
from oracle import per_view_oracle as pvo

ALL = kc.PAIR_CASES
KINDS = ("pose", "intrinsics")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "starst3r_amd", "csrc")
OLD_BAR = 1e-6          # test_gpu_pose_grad / test_gpu_intrinsics_grad: of the camera's largest entry


# ---- a. pair cases ----
@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_edge(oracle_built, name):
    R = kc.pair_reference(name)
    case = R["case"]
    case.check(case, R["O"])
    rec, v, vis = R["records"], R["v"], R["vis"]
    assert rec.shape == (case.Cn * case.N, 12) and v.shape == rec.shape
    # a culled pair: NaN in all twelve cotangents and in every float of its record but the radius word, which is integer 0
    assert np.isnan(v[~vis]).all() and np.isfinite(v[vis]).all()
    assert np.isnan(np.delete(rec[~vis], 10, axis=1)).all() and not rec[~vis, 10].view(np.int32).any()
    assert np.isfinite(rec[vis]).all() and (rec[vis, 10].view(np.int32) > 0).all()
    if name in pc.CASES:                             # the shared reference of the projection tests is left as it was
        assert not pc.reference(name)["O"]["records"][~vis].any()


@pytest.mark.parametrize("name", ALL)
def test_oracle_is_the_operation(oracle_built, name):
    """finisher(sum of the float64 pair terms) against float64 autograd into viewmats (campos = inverse(V)[:3, 3] inside
    the graph) and into (fx, fy, cx, cy): 1e-10 of the entry scale S, and exact zeros where S is 0"""
    R = kc.pair_reference(name)
    for kind in KINDS:
        K = R[kind]
        S, d = K["S"], np.abs(K["t64"] - K["r64"])
        assert np.isfinite(K["r64"]).all() and np.isfinite(K["o32"]).all()
        assert (d <= 1e-10 * S).all(), (name, kind, float((d[S > 0] / S[S > 0]).max()))
        assert not K["r64"][S == 0].any() and not K["o32"][S == 0].any()
        assert (np.abs(K["r64"]) <= S * (1 + 1e-12)).all()
    if R["case"].N:                                  # a camera's four intrinsics entries have a scale exactly if it sees a pair
        sees = R["vis"].reshape(R["case"].Cn, -1).any(1)
        assert np.array_equal((R["intrinsics"]["S"] > 0).all(1), sees) and np.array_equal((R["intrinsics"]["S"] > 0).any(1), sees)
        assert (R["pose"]["S"] > 0).any()


def test_bounds_come_from_the_float32_oracle(oracle_built):
    """bound = 4 max(own32 of the case, median own32 over all cases) S per entry; no case above FLOOR without saying why;
    the docstring table of per_view_kernel_cases holds what is measured here; against the old bar (1e-6 of the camera's
    largest entry) per case: the largest bound / old bar over the small entries (|ref| <= 0.1 max |ref|) and the others"""
    for kind in KINDS:
        rel = kc.rel_bounds(kind)
        med = kc._rel[kind + "_median"]
        for name in ALL:
            own = kc.pair_reference(name)[kind]["own32"]
            assert rel[name] == 4.0 * max(own, med)
            assert rel[name] <= kc.FLOOR or name in kc.ABOVE_FLOOR[kind], (kind, name, rel[name])
        assert not set(kc.ABOVE_FLOOR[kind]) - set(n for n in ALL if rel[n] > kc.FLOOR)
    table = own32_table()
    print(table)
    doc = {m.group(1): (float(m.group(2)), float(m.group(3)))
           for m in re.finditer(r"^\s+(\w+)\s+([\d.e+-]+)\s+([\d.e+-]+)\s", kc.__doc__, re.M) if m.group(1) in ALL}
    assert set(doc) == set(ALL)
    for name in ALL:
        for kind, written in zip(KINDS, doc[name]):
            own = kc.pair_reference(name)[kind]["own32"]
            assert abs(written - own) <= 0.06 * own + 1e-30, (name, kind, written, own)


def own32_table():
    lines = ["%-18s %-9s %-9s %-16s %-16s" % ("case", "pose", "intrinsics", "pose new/old", "intrinsics new/old")]
    for name in ALL:
        R = kc.pair_reference(name)
        cells = []
        for kind in KINDS:
            K, rel = R[kind], kc.rel_bounds(kind)[name]
            Cn = R["case"].Cn
            r, S = np.abs(K["r64"]).reshape(Cn, -1), K["S"].reshape(Cn, -1)
            big = r.max(1, keepdims=True)
            ok = big[:, 0] > 0
            if not ok.any():
                cells.append("-")
                continue
            ratio = (rel * S / (OLD_BAR * np.where(big > 0, big, 1.0)))[ok]
            small = (r <= 0.1 * big)[ok]
            cells.append("%.2f / %.2f" % (ratio[small].max() if small.any() else 0.0, ratio[~small].max()))
        lines.append("%-18s %-9.1e %-9.1e  %-16s %-16s" % (name, R["pose"]["own32"], R["intrinsics"]["own32"], *cells))
    lines.append("median             %-9.1e %-9.1e" % (kc._rel["pose_median"], kc._rel["intrinsics_median"]))
    return "\n".join(lines)


def test_every_clamp_side_reaches_both_kernels(oracle_built):
    """the clamped pairs counted from float64 (project_cases.clamp_sides) are the pairs on which the oracle takes the `else`
    branches, in both precisions; each side has its case with eight or more of them in the planted camera"""
    for side in ("xp", "xn", "yp", "yn"):
        name = "clamp_" + side
        R = kc.pair_reference(name)
        case = R["case"]
        sides, _ = pc.clamp_sides(case, R["O"])
        assert int(sides[side][0].sum()) >= 8
        i32, i64 = branches(name)
        pid = np.nonzero(R["vis"])[0]
        x_out = (sides["xp"] | sides["xn"]).reshape(-1)[pid]; y_out = (sides["yp"] | sides["yn"]).reshape(-1)[pid]
        for info in (i32, i64):
            assert np.array_equal(~info["x_in"], x_out) and np.array_equal(~info["y_in"], y_out)
        # the `else` terms weigh: without them the float64 sum moves by ten times the bound or more
        K = R["intrinsics"]
        col = 2 if side[0] == "x" else 3
        t64 = pvo.intrinsics_pair_terms(case, R["records"], R["v"], np.float64)
        plain = R["v"][pid, 0 if col == 2 else 1].astype(np.float64)
        moved = abs(pvo.camera_sums(t64[:, col:col + 1] - plain[:, None], R["cam"], case.Cn)[0, 0])
        assert moved > 10 * kc.rel_bounds("intrinsics")[name] * K["S"][0, col], (name, moved)


def branches(name):
    R = kc.pair_reference(name)
    i32, i64 = {}, {}
    pvo.pose_pair_terms(R["case"], R["records"], R["v"], np.float32, info=i32)
    pvo.pose_pair_terms(R["case"], R["records"], R["v"], np.float64, info=i64)
    return i32, i64


NEAR_A_LIMIT = {"regulariser_n1000": "one of 1988 random pairs lies 3.7e-5 relative from lim_x: 600 float32 units, and both "
                                     "precisions put it on the same side (asserted)"}


@pytest.mark.parametrize("name", ALL)
def test_branch_margins(oracle_built, name):
    """no visible pair within 1e-4 relative of a clamp limit or of a colour pre-clamp of 0 (the kernel's FMA contraction
    moves either by a few float32 units: 1e-7), and both precisions take the same branches on every pair"""
    R = kc.pair_reference(name)
    if R["case"].N == 0:
        return
    i32, i64 = branches(name)
    for k in ("x_in", "y_in", "colour_pass"):
        assert np.array_equal(i32[k], i64[k]), (name, k)
    _, near = pc.clamp_sides(R["case"], R["O"])
    assert near > (1e-5 if name in NEAR_A_LIMIT else 1e-4), (name, near)
    assert (name in NEAR_A_LIMIT) == (near <= 1e-4)
    assert float(i64["colour_margin"].min()) > 1e-4 and float(i32["colour_margin"].min()) > 1e-4
    if name == "colour_clamp":
        assert int((~i64["colour_pass"]).sum()) >= 24 and int(i64["colour_pass"].sum()) >= 24


def test_new_cases_cover_what_they_name(oracle_built):
    # trip2: 257 blocks (asserted by its predicate with the blocks that hold live pairs); the second trip of the finishers
    # holds exactly one partial
    assert -(-kc.TRIP2_N // 256) - pvo.STREAM_T == 1
    # cancel: v_t.x, v_t.y, v_cx, v_cy are sums of cancelling terms
    R = kc.pair_reference("cancel")
    P, I = R["pose"], R["intrinsics"]
    for S, r in ((P["S"][0, 0, 3], P["r64"][0, 0, 3]), (P["S"][0, 1, 3], P["r64"][0, 1, 3]), (I["S"][0, 2], I["r64"][0, 2]),
                 (I["S"][0, 3], I["r64"][0, 3])):
        assert S / abs(r) > 1e3, (S, r)
    # similarity_V, general_row3: row 3 of v_viewmats is not zero and has a scale of its own
    for name in ("similarity_V", "general_row3"):
        P = kc.pair_reference(name)["pose"]
        assert (P["S"][0, 3] > 0).all() and (np.abs(P["r64"][0, 3]) > 0).all()
    g = kc.pair_reference("general_row3")["pose"]
    rigid = kc.get("general_row3").viewmats[0].astype(np.float64).copy()
    rigid[3] = [0, 0, 0, 1]
    sums = g["sums64"][0]
    moved = np.abs(pvo.pose_finish(sums, rigid) - g["t64"][0])                  # row 3 of V matters: ten bounds or more
    assert (moved > 10 * kc.rel_bounds("pose")["general_row3"] * g["S"][0]).all()
    # dead_camera: the middle camera's scale is zero in every entry, its neighbours' is not
    D = kc.pair_reference("dead_camera")
    for kind in KINDS:
        assert not D[kind]["S"][1].any() and not D[kind]["r64"][1].any() and D[kind]["S"][0].any() and D[kind]["S"][2].any()
    # n0
    Z = kc.pair_reference("n0")
    assert Z["pose"]["r64"].shape == (2, 4, 4) and not Z["pose"]["S"].any() and not Z["intrinsics"]["S"].any()
    # row 3 of v_viewmats is tested on every camera that is not at the origin
    assert sum(int((kc.pair_reference(n)["pose"]["S"][:, 3] > 0).all(1).sum()) for n in ALL) > 300


def test_pair_cases_include_every_projection_case():
    assert ALL[:len(pc.CASES)] == list(pc.CASES) and ALL[len(pc.CASES):] == list(kc.NEW_CASES)
    assert "views_c256" in ALL and "sh_stride_72" in ALL and kc.get("views_c256").Cn == 256
    src = open(os.path.join(os.path.dirname(CSRC), "..", "include", "st3r.h")).read()
    assert re.search(r"#define ST3R_MAX_VIEWS 256\b", src)


# ---- b. stream shapes ----
def test_host_formulas_are_those_of_the_library():
    src = open(os.path.join(CSRC, "per_view.h")).read()
    assert re.search(r"#define STREAM_T 256\b", src) and re.search(r"#define STREAM_ALIGN 1024\b", src)
    assert "int64_t want = (C * HW + STREAM_ALIGN - 1) / STREAM_ALIGN;" in src
    assert "if (want > 256 * 8) want = 256 * 8;" in src and "int64_t b = want / C;" in src and "if (b < 1) b = 1;" in src
    assert "int64_t ch = (HW + b - 1) / b;" in src and "ch = (ch + STREAM_ALIGN - 1) / STREAM_ALIGN * STREAM_ALIGN;" in src
    assert "*blocks = (int)((HW + ch - 1) / ch);" in src
    assert "lo = (int64_t)blockIdx.x * chunk; hi = min(HW, lo + chunk);" in src
    assert "for (int b = threadIdx.x; b < n_part; b += STREAM_T)" in src and "#define WEIGHT_SUM_BORDER 5" in src
    for f, n in (("gs_exposure.hip", 2), ("loss_depth.hip", 2)):
        assert open(os.path.join(CSRC, f)).read().count("HW % 4 == 0 && aligned16(") == n
    assert (pvo.STREAM_T, pvo.STREAM_ALIGN, pvo.STREAM_MAX_WG) == (256, 1024, 2048)
    G = lambda C, HW: pvo.stream_grid(C, HW)[:2]
    assert G(1, 1) == (1, 1024) and G(1, 1024) == (1, 1024) and G(1, 1025) == (2, 1024) and G(1, 2048) == (2, 1024)
    assert G(1, 2049) == (3, 1024)
    assert G(2, 1024) == (1, 1024) and G(2, 1025) == (1, 2048)              # want = 3: 1 per view
    assert G(256, 16) == (1, 1024)                                           # want / C == 0 -> 1
    assert G(1, 2048 * 1024) == (2048, 1024) and G(1, 2048 * 1024 + 1) == (1025, 2048)     # the cap, on both sides
    assert G(3, 768 * 1024) == (384, 2048)                                   # test_gpu_exposure's capped shape
    assert pvo.vec(1056, True) and not pvo.vec(1056, False) and not pvo.vec(1035, True)
    assert pvo.trips(1024, True) == 1 and pvo.trips(1025, True) == 2 and pvo.trips(256, False) == 1 and pvo.trips(257, False) == 2


def test_stream_shapes_reach_what_the_table_says():
    T = {s: kc.shape_tags(s) for s in kc.STREAM_SHAPES}
    t = T[(1, 45, 23)]
    assert (t["vec"], t["blocks"], t["trips"], t["last"]) == (False, 2, 4, 11)
    t = T[(2, 33, 63)]
    assert (t["vec"], t["chunk"], t["trips"], t["blocks"], t["last"], t["odd_base"]) == (False, 2048, 8, 2, 31, True)
    t = T[(3, 33, 32)]
    assert (t["vec"], t["blocks"], t["trips"], t["last_live_threads"]) == (True, 1, 2, 8)
    t = T[(1, 1, 1028)]
    assert (t["vec"], t["blocks"], t["last"], t["last_live_threads"]) == (True, 2, 4, 1)
    t = T[(8, 120, 160)]
    assert (t["vec"], t["blocks"], t["trips"], t["short_last"], t["last"]) == (True, 10, 2, True, 768)
    assert T[(256, 4, 4)]["want_zero"] and T[(256, 4, 4)]["blocks"] == 1
    t = T[(1, 257, 1024)]
    assert (t["blocks"], t["wraps"], t["cap"]) == (257, True, False) and 257 > 5 + 10       # an interior of 247 x 1014
    t = T[(1, 2049, 1024)]
    assert (t["cap"], t["blocks"], t["chunk"], t["wraps"]) == (True, 1025, 2048, True)
    # the tag set
    tags = list(T.values()) + [kc.shape_tags(s, aligned=False) for s in kc.STREAM_SHAPES]
    assert any(t["vec"] for t in tags) and any(not t["vec"] for t in tags)
    for v in (True, False):
        assert any(t["vec"] == v and t["blocks"] > 1 and t["trips"] > 1 for t in tags)
        assert any(t["vec"] == v and t["short_last"] for t in tags)
        assert any(t["vec"] == v and t["wraps"] for t in tags)
    assert any(t["want_zero"] for t in tags) and any(t["cap"] for t in tags)
    assert kc.EXPOSURE_SHAPES == kc.STREAM_SHAPES[:-1]
    assert all(not t["cap"] for s, t in T.items() if s in kc.EXPOSURE_SHAPES)


def exact_sum(a):
    """the sum of a 1-D float64 array if adding it forwards, backwards and in extended precision all give math.fsum's
    correctly rounded result, else an assertion"""
    a = np.asarray(a, np.float64).reshape(-1)
    want = math.fsum(a.tolist())
    fwd = float(np.cumsum(a)[-1]) if a.size else 0.0
    bwd = float(np.cumsum(a[::-1])[-1]) if a.size else 0.0
    ext = float(a.astype(np.longdouble).sum())
    assert fwd == want and bwd == want and ext == want and float(a.sum()) == want, (fwd, bwd, ext, want)
    return want


@pytest.mark.parametrize("shape", kc.STREAM_SHAPES)
def test_dyadic_inputs_add_up_exactly_in_any_order(shape):
    C, H, W = shape
    if shape in kc.EXPOSURE_SHAPES:
        x, vy, E = kc.exposure_inputs(shape)
        assert np.array_equal(x * 16, np.round(x * 16)) and x.min() >= 0 and x.max() <= 1
        assert np.array_equal(vy * 8, np.round(vy * 8)) and np.abs(vy).max() <= 2 and np.array_equal(E * 8, np.round(E * 8))
        y, vx, vE = kc.exposure_reference(x, vy, E)
        # y and v_x are float32 numbers, and float32 arithmetic in the kernel's two orders gives them
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.array_equal(vx.astype(np.float32), vx)
        A, t = E[:, :, :3], E[:, :, 3]
        chain = t[:, None, None, :] + A[:, None, None, :, 0] * x[..., 0:1]
        chain = chain + A[:, None, None, :, 1] * x[..., 1:2]
        chain = chain + A[:, None, None, :, 2] * x[..., 2:3]
        assert chain.dtype == np.float32 and np.array_equal(chain, y)
        for c in range(C):
            for j in range(3):
                for i in range(3):
                    assert exact_sum(vy[c, :, :, j].astype(np.float64) * x[c, :, :, i]) == vE[c, j, i]
                assert exact_sum(vy[c, :, :, j]) == vE[c, j, 3]
    D, alpha, Z, w, tie = kc.depth_inputs(shape)
    ref = kc.depth_reference(D, alpha, Z, w)
    on = w > 0
    assert np.isin(alpha, np.array([1.0, 0.5, 0.25, 0.0, 5e-11], np.float32)).all()
    assert not np.isfinite(Z[~on]).any() and np.isfinite(Z[on]).all() and np.isfinite(D).all()
    assert np.isnan(w).any() or C * H * W < 200
    assert (w < 0).any() or C * H * W < 200
    assert tie.any() and (ref["ed"][tie] == Z[tie]).all() and not ref["v_depth"][tie].any() and not ref["terms"][tie].any()
    low = alpha < kc.DP_MIN_ALPHA
    assert (low & on & (D > 0)).any() and not ref["v_alpha"][low].any() and ref["v_depth"][low & on & ~tie].any()
    if C > 1:
        assert not on[C - 1].any() and ref["n_c"][C - 1] == 1.0 and ref["sums"][C - 1] == 0.0
    assert np.isfinite(ref["v_depth"]).all() and np.isfinite(ref["v_alpha"]).all()
    assert not ref["v_depth"][~on].any() and not ref["v_alpha"][~on].any()
    for c in range(C):
        assert exact_sum(ref["terms"][c]) == ref["sums"][c]
        assert max(exact_sum(ref["w64"][c]), 1.0) == ref["n_c"][c]
    n1, n2, w64 = kc.weight_sums_reference(w)
    for c in range(C):
        assert max(exact_sum(w64[c]), 1.0) == n1[c]
        if H > 10 and W > 10:
            assert max(exact_sum(w64[c, 5:H - 5, 5:W - 5]), 1.0) == n2[c]
        else:
            assert n2[c] == 1.0


# ---- c. Adam ----
def test_adam_moments_exact_is_adam():
    rng = np.random.default_rng(5)
    m = (0.01 * rng.standard_normal(200)).astype(np.float32); v = (1e-4 * rng.uniform(0, 1, 200)).astype(np.float32)
    g = rng.standard_normal(200)
    differ = 0
    for b1, b2 in kc.ADAM_BETAS:
        a = pvo.adam_moments_exact(m, v, g, b1, b2, False)
        b = pvo.adam_moments_exact(m, v, g, b1, b2, True)
        pm = b1 * m.astype(np.float64) + (1 - b1) * g
        pv = b2 * v.astype(np.float64) + (1 - b2) * g * g
        for got in (a, b):
            assert (np.abs(got[0] - pm) <= np.spacing(np.abs(pm).astype(np.float32))).all()
            assert (np.abs(got[1] - pv) <= np.spacing(np.abs(pv).astype(np.float32))).all()
        assert np.array_equal(a[1], b[1])                            # the second moment does not depend on M_LAST
        differ += int((a[0] != b[0]).sum())
        if b1 == 0.0:                                                # beta 0: m = g, v = g^2 rounded once
            assert np.array_equal(a[0], g.astype(np.float32)) and np.array_equal(a[1], (g * g).astype(np.float32))
    print("M_LAST changes %d of 600 stored first moments" % differ)
    # zero in, zero out
    z = np.zeros(3, np.float32)
    mo, vo = pvo.adam_moments_exact(z, z, np.zeros(3), 0.9, 0.999, False)
    assert not mo.any() and not vo.any()


@pytest.mark.parametrize("kind", ["exposure", "intrinsics", "pose"])
def test_adam_cases_cover_what_they_name(kind):
    swaps = 0
    for C in kc.ADAM_C:
        mask = kc.adam_mask(C)
        assert mask[0] == 1.0 and (C < 4 or (mask[1] == 0 and np.signbit(mask[2]) and mask[2] == 0 and mask[3] == np.float32(1e-30)))
        assert mask[3 % C] != 0 or C == 1
        for betas in kc.ADAM_BETAS:
            for step in kc.ADAM_STEPS:
                A = kc.adam_case(kind, C, betas, step)
                assert np.array_equal(A["frozen"], mask == 0)
                if C >= 4:
                    fz = np.nonzero(A["frozen"])[0]
                    assert np.signbit(A["m"][fz, 0]).all() and np.signbit(A["grad"].reshape(C, -1)[fz, 1]).all()
                if step == 1:
                    z = A["zero"]
                    assert not A["frozen"][z] and not A["grad"][z].any() and not A["m"][z].any() and not A["v"][z].any()
                if kind != "pose" and betas[0] == 0.9:            # a swapped M_LAST shows in the stored bits of the planted slots
                    g = A["grad"].reshape(C, -1).astype(np.float64) * (1.0 if kind == "exposure" else [1, 1, kc.ADAM_W, kc.ADAM_H])
                    a = pvo.adam_moments_exact(A["m"], A["v"], g, *betas, False)[0]
                    b = pvo.adam_moments_exact(A["m"], A["v"], g, *betas, True)[0]
                    live = int((~A["frozen"]).sum()) - (step == 1)
                    assert int(A["planted"].sum()) == live
                    hit = (np.abs(a - b) > 0.01 * np.abs(a))[A["planted"]]
                    assert hit.sum() >= 0.5 * live, (C, step, int(hit.sum()), live)
    if kind == "pose":
        for lr, angle in ((1.0, 1.73), (1.8, 3.12), (1e-9, 1.7e-9)):
            A = kc.adam_case("pose", 5, (0.9, 0.999), 1, zero_moments=True)
            *_, delta = kc.ref_pose_step(A["param"], A["grad"], A["m"], A["v"], lr, 0.9, 0.999, kc.ADAM_EPS, 1)
            live = [c for c in range(5) if c != A["zero"]]
            assert np.allclose(np.abs(delta[live, :3]), lr, rtol=1e-6)
            th = np.linalg.norm(delta[live, :3], axis=1)
            assert np.allclose(th, angle, rtol=5e-3) and ((th * th < 1e-16).all() == (lr == 1e-9)) and (th > 0).all()
            assert th.max() < math.pi
            assert not delta[A["zero"]].any()
