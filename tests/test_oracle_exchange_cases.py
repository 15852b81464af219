"""CPU pins of tests/exchange_cases.py -- the cases of test_gpu_exchange_cases.py -- with numpy and the C oracle alone (no
GPU): the restated host arithmetic is the source's, the case lists reach every piece, tail, range and block edge they
name, the references are what they claim to be.  A retuned condition or a thinned list fails here."""
import os
import re

import numpy as np
import pytest

import exchange_cases as xc
import loss_adam_cases as lac


def _src(name):
    with open(os.path.join(xc.CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


# ---- the restated host arithmetic is the source's ----
def test_kernel_choice_is_st3r_adam_impls_condition():
    s = _src("adam.hip")
    assert "const bool contiguous = !(g1 - g0 < N) && !gstage;" in s
    assert ("if (contiguous && N % 4 == 0 && i0 % 4 == 0 && (i1 - i0) % 4 == 0 && sh_stride % 4 == 0 && "
            "aligned16(means, quats, scales, opacities, sh, grads, m, v, pstage)) {") in s
    assert "if (total <= 0) return ST3R_OK;" in s
    # every clause of the condition decides on its own
    assert xc.adam_kernel(336, 1932, 3864) == "k_adam4"
    assert xc.adam_kernel(333, 1932, 3864) == "k_adam"                  # N % 4
    assert xc.adam_kernel(336, 966, 1932) == "k_adam"                   # i0 % 4
    assert xc.adam_kernel(336, 1932, 3862) == "k_adam"                  # (i1 - i0) % 4
    assert xc.adam_kernel(336, 1932, 3864, sh_stride=13) == "k_adam"
    assert xc.adam_kernel(336, 1932, 3864, sh_stride=12) == "k_adam4"
    assert xc.adam_kernel(336, 1932, 3864, aligned=False) == "k_adam"
    assert xc.adam_kernel(336, 1932, 3864, by_gaussian=True) == "k_adam"
    assert xc.adam_kernel(336, 0, 0) is None and xc.adam_kernel(2, 0, 0) is None


def test_pieces_tail_and_ranges_are_st3r_gs_train_steps():
    s = _src("comm.hip")
    assert s.count("const int64_t q = total / w, tail0 = q * w;") == 2          # rs_ag and direct
    assert "const int64_t total = (int64_t)23 * N;" in s
    assert s.count("r * q, (r + 1) * q, 0, -1,") == 2 and s.count("tail0, total, 0, -1, nullptr, nullptr, nullptr);") == 2
    assert "#define EXCH_RANGES_K 4" in s and xc.RANGES_K == 4
    assert "const int K = (mode == ST3R_EXCHANGE_RANGES && N >= 4096) ? EXCH_RANGES_K : 1;" in s and xc.RANGES_FROM == 4096
    assert s.count("const int64_t g0 = (int64_t)N * j / K, g1 = (int64_t)N * (j + 1) / K;") == 2
    assert xc.layout(1003, 4) == (23069, 5767, 23068)
    assert xc.pieces(1, 2) == [(0, 11), (11, 22)]
    assert xc.ranges(4095) == (1, [(0, 4095)])
    assert xc.ranges(4096) == (4, [(0, 1024), (1024, 2048), (2048, 3072), (3072, 4096)])
    assert xc.ranges(4099) == (4, [(0, 1024), (1024, 2049), (2049, 3074), (3074, 4099)])
    for N in xc.RANGE_NS:                       # the ranges tile [0, N); uneven wherever 4 does not divide N
        K, R = xc.ranges(N)
        assert R[0][0] == 0 and R[-1][1] == N and all(a[1] == b[0] for a, b in zip(R, R[1:]))
        assert (len({g1 - g0 for g0, g1 in R}) > 1) == (K > 1 and N % 4 != 0)
    assert [xc.ranges(N)[0] for N in xc.RANGE_NS] == [1, 4, 4, 4, 4]            # both sides of the switch


def test_bounds_are_test_gpu_adams():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_adam.py")) as f:
        s = f.read()
    assert "np.testing.assert_allclose(P[name], ref[name], rtol=0, atol=3e-7, err_msg=name)" in s and xc.PARAM_ATOL == 3e-7
    assert "np.testing.assert_allclose(m, m_o, rtol=1e-5, atol=1e-12)" in s and (xc.M_RTOL, xc.M_ATOL) == (1e-5, 1e-12)
    assert "np.testing.assert_allclose(v, v_o, rtol=1e-5, atol=1e-20)" in s and (xc.V_RTOL, xc.V_ATOL) == (1e-5, 1e-20)


def test_buffer_layout_is_loss_adam_cases():
    for N in (1, 5, 336):
        st = xc.block_starts(N)
        assert st == [0, 3 * N, 7 * N, 10 * N, 11 * N, 23 * N]
        sl = lac.adam_block_slices(N)
        assert [sl[k].start for k, _ in xc.BLOCKS] == st[:-1]
        assert xc.block_of(N, 0) == (0, 0) and xc.block_of(N, 23 * N - 1) == (4, 12 * N - 1) and xc.block_of(N, 11 * N) == (4, 0)
    rng = np.random.default_rng(0)
    buf = rng.standard_normal(23 * 7).astype(np.float32)
    assert np.array_equal(xc.pack(xc.unpack(buf)), buf)
    g = xc.piece_gaussians(7, 3)
    p = xc.pack(g)
    assert np.array_equal(p[:21], g["means"].ravel()) and np.array_equal(p[11 * 7:], g["shN"][:, :4].ravel())


# ---- part 1: the case list as a whole ----
EXPECT = {   # (N, w): (total, q, tail) of the issue's table
    (1, 2): (23, 11, 1), (1, 4): (23, 5, 3), (1, 8): (23, 2, 7), (3, 64): (69, 1, 5), (2, 64): (46, 0, 46),
    (336, 3): (7728, 2576, 0), (336, 4): (7728, 1932, 0), (336, 8): (7728, 966, 0), (1003, 4): (23069, 5767, 1)}


def test_piece_cases_are_the_listed_ones():
    listed = [(1, 2), (1, 4), (1, 8), (3, 64), (2, 64), (5, 3), (333, 7), (336, 3), (336, 4), (336, 8), (1003, 4)]
    assert xc.PIECE_CASES[:len(listed)] == listed and len(set(xc.PIECE_CASES)) == len(xc.PIECE_CASES)
    for (N, w), (total, q, tail) in EXPECT.items():
        t, qq, tail0 = xc.layout(N, w)
        assert (t, qq, t - tail0) == (total, q, tail), (N, w)


def test_kernel_tags():
    tags = {c: xc.piece_tags(*c) for c in xc.PIECE_CASES}
    assert all(t["kernel"] == "k_adam4" for t in tags[(336, 3)])
    assert all(t["kernel"] == "k_adam4" for t in tags[(336, 4)]) and tags[(336, 4)][1]["i0"] == 1932
    assert all(t["kernel"] == "k_adam" for t in tags[(336, 8)])               # q = 966: scalar although N % 4 == 0
    assert all(t["kernel"] is None for t in tags[(2, 64)]) and tags[(2, 64)][0]["tail_kernel"] == "k_adam"
    assert all(t["tail_kernel"] is None for c in ((336, 3), (336, 4), (336, 8)) for t in tags[c])
    for c in xc.PIECE_CASES:
        if c[0] % 4:
            assert all(t["kernel"] in ("k_adam", None) for t in tags[c]), c
    # the two additional runs of (336, 4): a stage 4 bytes off takes the scalar kernel, the compact SH tensor stays four-wide
    assert all(t["kernel"] == "k_adam" for t in xc.piece_tags(336, 4, aligned=False))
    assert all(t["kernel"] == "k_adam4" for t in xc.piece_tags(336, 4, sh_stride=12))
    # both kernels occur with i0 > 0
    seen = {t["kernel"] for ts in tags.values() for t in ts if t["i0"] > 0}
    assert {"k_adam", "k_adam4"} <= seen


def test_boundaries_reach_every_block_and_edge():
    B = [(c, b) for c in xc.PIECE_CASES for b in xc.boundaries(*c)]
    for name, _ in xc.BLOCKS:                                   # some boundary strictly inside each of the five blocks
        assert any(b["block"] == name and b["inside"] for _, b in B), name
    assert any(b["sh_pos"] not in (None, 0) for _, b in B)      # inside a Gaussian's twelve SH scalars
    assert any(b["on_block_start"] for _, b in B)               # exactly on a block boundary
    assert {"at": 11, "block": "shN", "inside": False, "on_block_start": True, "sh_pos": 0} in xc.boundaries(1, 2)
    assert xc.boundaries(2, 64) == []                           # q = 0: nothing but tail
    # the same with the k_adam4 cases alone: its float4 groups meet a piece boundary inside the SH block
    assert any(b["block"] == "shN" and b["inside"] for c, b in B if c in ((336, 3), (336, 4)))
    for (N, w), b in B:
        assert 0 < b["at"] < 23 * N


def test_every_tail_length_occurs():
    for w in (8,):
        tails = {23 * N - xc.layout(N, ww)[2] for N, ww in xc.PIECE_CASES if ww == w}
        assert tails == set(range(w)), (w, tails)
    assert any(xc.layout(*c)[1] == 0 for c in xc.PIECE_CASES)   # an empty piece
    # part 3: every tail length 0 .. w - 1 for each world, and the tails worked out in the issue
    Ns = [n for _, n, _ in xc.WORLD_CASES]
    for w in xc.WORLDS:
        assert {23 * n % w for n in Ns} == set(range(w)), w
    assert [23 * 1 % w for w in xc.WORLDS] == [1, 2, 3]
    assert [23 * 4096 % w for w in xc.WORLDS] == [0, 2, 0]
    assert [23 * 4097 % w for w in xc.WORLDS] == [1, 1, 3]
    q = {w: xc.layout(4096, w)[1] for w in xc.WORLDS}
    assert q[2] % 4 == 0 and q[4] % 4 == 0 and q[3] % 4 != 0
    assert {t["kernel"] for t in xc.piece_tags(4096, 2) + xc.piece_tags(4096, 4)} == {"k_adam4"}
    assert {t["kernel"] for t in xc.piece_tags(4096, 3)} == {"k_adam"}


def test_world_cases_are_the_listed_ones():
    assert [n for _, n, a in xc.WORLD_CASES if not a] == [1, 2, 3, 5, 4095, 4096, 4097, 4098, 4099]
    assert [(n, a) for _, n, a in xc.WORLD_CASES if a] == [(5, True)]
    assert xc.WORLDS == (2, 3, 4) and xc.RANGE_NS == (4095, 4096, 4097, 4098, 4099) and (xc.VIEW_W, xc.VIEW_H) == (48, 32)
    assert len({name for name, _, _ in xc.WORLD_CASES}) == len(xc.WORLD_CASES)


# ---- references ----
def test_foreign_moments_are_nonzero_exactly_where_the_rank_owns_nothing():
    for N, w in xc.PIECE_CASES:
        for r in (0, w // 2, w - 1):
            m, v, keep = xc.foreign_moments(N, w, r, 5)
            assert np.array_equal(keep, ~xc.owned(N, w, r))
            assert not m[~keep].any() and not v[~keep].any() and (m[keep] != 0).all() and (v[keep] > 0).all()


def test_piece_reference_is_the_oracle_on_the_whole_buffer(oracle_built):
    R = xc.piece_reference(5, 3)
    g0 = R["g0"]
    assert g0["shN"].shape == (5, 24, 3) and np.abs(g0["shN"][:, 4:]).min() > 0
    (gr1, P1, m1, v1), (gr2, P2, m2, v2) = R["steps"]
    assert np.array_equal(P2["shN"][:, 4:].view(np.int32), g0["shN"][:, 4:].view(np.int32))
    # step 1 from zero moments: m is the rounded product, the step is lr * sign(g) to 1e-5
    assert np.array_equal(m1.view(np.int32), xc.first_moment_bits(gr1))
    d = xc.pack(P1).astype(np.float64) - xc.pack(g0)
    big = np.abs(gr1) > 1e-4
    assert np.allclose(d[big], -1e-3 * np.sign(gr1[big]), rtol=0, atol=2e-7)
    assert not np.array_equal(m2, m1) and (v2 >= 0).all()
    p, m, v = xc.oracle_step(xc.pack(P1), m1, v1, gr2, 2)       # the packed wrapper is the same oracle
    assert np.array_equal(p, xc.pack(P2)) and np.array_equal(m, m2) and np.array_equal(v, v2)
    assert xc.piece_reference(336, 4, compact_sh=True)["g0"]["shN"].shape == (336, 4, 3)
    assert xc.over_bounds(p, m, v, p, m, v) == (0.0, 0.0, 0.0)
    assert xc.over_bounds(p + np.float32(6e-7), m, v, p, m, v)[0] > 1.0


def test_first_moment_bits_is_one_rounded_product():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    S = lac.wide_range_grads(rng, 4000)
    S[:4] = [0.0, -0.0, 1e-30, -3.0]
    got = xc.first_moment_bits(S)
    w1 = Fraction(float(np.float32(0.1)))
    assert np.float32(1.0 - 0.9) == np.float32(0.1)
    for i in range(0, 4000, 7):
        exact = w1 * Fraction(float(S[i]))
        assert np.float32(float(exact)).view(np.int32) == got[i] or abs(float(exact)) < 1e-37   # (float(Fraction) rounds once)
    assert got[0] == 0 and got[1] == 0                           # +0 from either zero
    a = np.array([1.0, 2.0 ** -24, -1.0], np.float32)
    assert np.array_equal(xc.rank_ordered_sum([a[:1], a[1:2], a[1:2]]), np.array([1.0], np.float32))   # (1 + e) + e = 1
    assert xc.rank_ordered_sum([a[1:2], a[1:2], a[:1]])[0] > 1.0                                       # (e + e) + 1 > 1


def test_scenes_put_every_rank_in_front_of_something(oracle_built):
    """every rank's 48 x 32 view sees at least one Gaussian; the turned-away camera sees none"""
    from oracle import gs_oracle as go
    for w in xc.WORLDS:
        for name, N, away in xc.WORLD_CASES:
            g, w2c, Ks, gt = xc.scene(N, w, away)
            assert w2c.shape == (w, 4, 4) and gt.shape == (w, xc.VIEW_H, xc.VIEW_W, 3) and g["shN"].shape == (N, 24, 3)
            pr = go.project_packed(g["means"], g["quats"], g["scales"], w2c, Ks, xc.VIEW_W, xc.VIEW_H)
            seen = np.bincount(pr["camera_ids"], minlength=w)
            assert (seen[:w - 1] > 0).all(), (w, name, seen)
            assert (seen[w - 1] == 0) if away else (seen[w - 1] > 0), (w, name, seen)
    g, w2c, Ks, gt = xc.scene(4097, 1)
    assert w2c.shape == (1, 4, 4)
