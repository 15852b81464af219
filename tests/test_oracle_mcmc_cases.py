"""CPU pins of tests/mcmc_cases.py -- the inputs of test_gpu_mcmc_cases.py -- with oracle/mcmc_oracle.py alone (no GPU):
every case plants what it names (asserted on the oracle's own values), the exact weights are what a float32 sigmoid
gives, the bounds behave as derived, and the domain of the float32 relocation formula is tabulated."""
import numpy as np
import pytest

import mcmc_cases as mc
from oracle import mcmc_oracle as mo

F = np.float32


def test_the_three_logits_have_exact_sigmoids():
    assert (mo.sigmoid32(np.arange(17, 21, dtype=F)) == 1.0).all()
    assert (mo.sigmoid32(-np.arange(89, 201, dtype=F)) == 0.0).all()
    assert mo.sigmoid32(F(0)) == 0.5
    for lg in (17.0, 20.0, -200.0):      # and expf(-0) == 1 exactly
        assert mc.sigmoid_is_robust(F(lg))


@pytest.mark.parametrize("N", mc.EXACT_N)
def test_exact_case_plants_what_it_names(N):
    c = mc.exact_case(N)
    lg, w = c["P"]["opacities"], c["w"]
    w_o, dead_o = mo.weights(lg, c["min_opacity"], True)
    np.testing.assert_array_equal(w_o, w)                      # relocating: only the zeros are dead
    np.testing.assert_array_equal(dead_o, w == 0)
    np.testing.assert_array_equal(mo.weights(lg, c["min_opacity"], False)[0], w)
    assert set(np.unique(w)) <= {0, 1 << 23, 1 << 24}
    if N >= 255:
        assert set(np.unique(w)) == {0, 1 << 23, 1 << 24} and w[0] == 0 and w[N - 1] == 0
    for e in range(mc.TILE, N + 1, mc.TILE):                   # both sides of every tile edge
        assert w[e - 1] == 0 and (e == N or w[e] == 0)
    if N >= 2047:
        assert (w[900:1200] == 0).all() and w[899] != 0 and w[1200] != 0
    cum = np.cumsum(w, dtype=np.uint64)
    if N >= 2047:
        assert cum[-1] > 1 << 32 and int(np.searchsorted(cum, 1 << 32)) < 600
    n_tiles = -(-N // mc.TILE)
    assert (n_tiles > 256) == (N == 524289) and (N != 524288 or n_tiles == 256)
    n_dead = int((w == 0).sum())
    assert n_dead <= 900 and c["n_new"] <= 200
    if N > 2:
        Q = {k: v.copy() for k, v in c["P"].items()}
        ids, sampled = mo.relocate(Q, None, c["min_opacity"], seed=c["seed"], step=c["step"])
        assert len(ids) == n_dead and (w[sampled] > 0).all()
        assert np.bincount(sampled).max() <= 12              # small ratios: well inside the formula's domain
        uniq, counts = np.unique(sampled, return_counts=True)
        for g, k in zip(uniq[:40], counts[:40]):
            assert mc.reloc_bound(lg[g], c["P"]["scales"][g], int(k) + 1, c["min_opacity"])["in_domain"]


def test_plateau_case():
    lg = mc.plateau_logits()
    w = mc.exact_weights(lg)
    np.testing.assert_array_equal(mo.weights(lg, 0.005, False)[0], w)
    assert w[0] == 0 and w[1] != 0 and (w[60:] == 0).all() and w[59] != 0 and (w[40:52] == 0).all() and (w[9:13] == 0).all()
    cum = np.cumsum(w, dtype=np.uint64)
    s = mo.draw(cum, np.arange(4096), mo.STREAM_ADD, 3, (9 << 32) | 5)
    assert (w[s] > 0).all() and len(np.unique(s)) == int((w > 0).sum())   # every positive weight is drawn, no zero is
    # all weights zero: every draw is clamped to N - 1
    z = np.zeros(64, np.uint64)
    assert (mo.draw(z, np.arange(5), mo.STREAM_ADD, 1, 1) == 63).all()
    P = mc.params(64, np.full(64, mc.L_ZERO), seed=3)
    with np.errstate(all="ignore"):
        grown, s = mo.add_new(P, 5, 0.005, seed=1, step=1)
    assert np.isnan(grown["scales"][63:]).all()
    assert grown["opacities"][63] == np.log(F(0.005) / (F(1) - F(0.005)), dtype=F)


def test_tiny_weights_make_draws_land_on_prefix_sums():
    lg = mc.tiny_logits()
    w, _ = mo.weights(lg, 0.005, False)
    assert set(np.unique(w)) == {0, 1, 5} and w[0] == 0 and w[63] == 0
    x = mo.sigmoid32(lg[w > 0]).astype(np.float64) * 2 ** 24            # far from an integer: an ulp does not move it
    assert (np.abs(x - np.rint(x)) > 0.1).all()
    cum = np.cumsum(w, dtype=np.uint64)
    s = mo.draw(cum, np.arange(2048), mo.STREAM_ADD, 2, 6)
    assert (w[s] > 0).all()
    # the same draws with the search taking the first prefix sum >= t instead of > t: a different source on every draw that equals a prefix sum (weights of 1: most of them)
    r0, r1, _, _ = mo.philox4x32_10(np.arange(2048, dtype=np.uint64), 0, mo.STREAM_ADD, 2, 6, 0)
    t = np.array([(((int(a) << 32) | int(b)) * int(cum[-1])) >> 64 for a, b in zip(r0, r1)], np.uint64)
    ge = np.minimum(np.searchsorted(cum, t, side="left"), 63)
    assert (ge != s).mean() > 0.3 and (w[ge] == 0).any()


def test_forced_ratios():
    for n_dead in (1, 4, 19, 48, 49, 50, 51, 69):
        P = mc.single_source(F(0.3), n_dead)
        ids, sampled = mo.relocate({k: v.copy() for k, v in P.items()}, None, 0.005, seed=4, step=2)
        assert len(ids) == n_dead and (sampled == 0).all()
    P = mc.two_sources()
    ids, sampled = mo.relocate({k: v.copy() for k, v in P.items()}, None, 0.005, seed=11, step=0)
    c = np.bincount(sampled, minlength=62)
    assert c[7] + c[40] == 60 and 0 < c[40] < c[7] and c[7] >= 51


def test_grid_bounds_and_domain_table():
    """The bound per (o, ratio); ratio-2 sources at mid opacity stay near 1e-6; the whole grid is inside the domain."""
    ls = np.array([-4.0, -3.5, -5.0], F)
    print()
    for o in mc.GRID_O:
        for r in mc.GRID_RATIO:
            lg = mc.logit_of(o)
            b = mc.reloc_bound(lg, ls, r, 0.005)
            print("o=%-12.9g ratio=%2d  oracle err: logit %.1e log-scale %.1e | floor %.1e %.1e | bound %.1e %.1e"
                  % (o, r, b["yard_logit"], b["yard_logscale"], b["floor_logit"], b["floor_logscale"],
                     b["bound_logit"], b["bound_logscale"]))
            assert b["in_domain"], (o, r)
            assert b["yard_logscale"] <= b["floor_logscale"] * 4            # the oracle itself obeys the error analysis
            assert b["yard_logit"] <= b["floor_logit"] * 4
    for o in (0.1, 0.5, 0.9):
        b = mc.reloc_bound(mc.logit_of(o), ls, 2, 0.005)
        assert b["bound_logscale"] < 5e-6 and b["bound_logit"] < 5e-6, (o, b)
    for o in (1 - 2.0 ** -13, 1 - 2.0 ** -23):
        assert mc.sigmoid_is_robust(mc.logit_of(o)) and float(mo.sigmoid32(mc.logit_of(o))) == o


def test_domain_of_the_float32_formula():
    """o == 1.0f (any logit >= 17): the float32 scale factor against float64, by ratio.  `in_domain` gives up at ratio
    25 (no correct digit); from ratio 32 on the float32 sum is negative (log -> NaN scale) -- upstream's arithmetic,
    recorded in DESIGN.md.  There the sign depends on how the sum is rounded: a fused multiply-add gives the other sign
    at ratios 32, 47, 49, 50, which is why the kernel switches contraction off and why the GPU pin holds those counts."""
    ls = np.zeros(3, F)
    first_out, rows = None, []
    for r in range(2, 52):
        b = mc.reloc_bound(F(20.0), ls, r, 0.005)
        with np.errstate(all="ignore"):
            _, s32 = mo.compute_relocation(np.array([1.0], F), np.ones((1, 3), F), np.array([r]))
        rows.append((r, float(s32[0, 0]), b["coeff"], b["floor_logscale"]))
        if first_out is None and not b["in_domain"]:
            first_out = r
        if b["in_domain"]:
            assert abs(float(s32[0, 0]) / b["coeff"] - 1) <= b["floor_logscale"]
    print()
    for r, s32, s64, fl in rows:
        print("o=1.0f ratio=%2d float32 %+.4e float64 %.4f floor %.1e" % (r, s32, s64, fl))
    assert first_out == 25
    assert all(r[1] > 0 for r in rows[:31 - 1]) and all(r[1] < 0 for r in rows[32 - 2:])
    differ = [n for n in range(25, 52)
              if (mc.denominator32_at_one(n, False) < 0) != (mc.denominator32_at_one(n, True) < 0)]
    assert differ == [32, 47, 49, 50]
    for n in (32, 40, 51):
        assert F(1) / F(mc.denominator32_at_one(n, False)) == F(rows[n - 2][1])         # the oracle's own sum
    assert rows[40 - 2][1] < 0 and 0.43 < rows[40 - 2][2] < 0.44        # ratio 40: -3.3e-4 against 0.433
    assert abs(rows[51 - 2][2] - 0.422) < 1e-3 and abs(rows[51 - 2][1]) < 1e-3
    for lg, cnt in ((20.0, 24), (20.0, 31), (20.0, 39), (17.0, 39), (20.0, 45), (20.0, 46), (20.0, 48), (20.0, 49),
                    (20.0, 50), (20.0, 69)):
        assert not mc.reloc_bound(F(lg), ls, cnt + 1, 0.005)["in_domain"]


def test_thresholds():
    w, dead = mo.weights(np.array([0.0, 1e-3, 3.0, -1e-3], F), 0.5, True)
    assert dead.tolist() == [True, False, False, True] and mo.sigmoid32(F(1e-3)) > 0.5
    b = mc.reloc_bound(F(1e-3), [-4, -3.5, -5], 3, 0.5)
    assert b["ref_logit"] == 0.0 and b["oracle_logit"] == 0.0          # the lower clamp
    b = mc.reloc_bound(F(20.0), [-4, -3.5, -5], 2, 0.005)
    assert b["oracle_logit"] == np.log(F(2.0 ** 23 - 1), dtype=F)        # the upper clamp


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_noise_case_and_bound(N):
    P = mc.noise_case(N)
    assert (P["means"] == 0).all()
    want, bound, yard, exact_zero = mc.noise_bound(P, 500.0, 9, (0xDEADBEEF << 32) | 5)
    arg = mc.gate_arg32(P["opacities"])
    assert not ((arg > 87.0) & (arg < 89.5)).any()
    with np.errstate(over="ignore"):
        assert (np.isinf(np.exp(arg[exact_zero], dtype=F))).all()
    f32 = mc.noise_f32(P["quats"], P["scales"], P["opacities"], 500.0, 9, (0xDEADBEEF << 32) | 5)
    assert (f32[exact_zero] == 0).all() and (f32[~exact_zero] != 0).any(1).all()
    if N >= 255:
        qn = np.linalg.norm(P["quats"], axis=1)
        assert qn.min() < 2e-3 and qn.max() > 500 and P["scales"].min() == -8 and P["scales"].max() == 1
        assert exact_zero.sum() > 50 and (~exact_zero).sum() > 100
        op = mo.sigmoid32(P["opacities"]).astype(np.float64)
        g = 1 / (1 + np.exp(-100 * ((1 - op) - 0.995)))
        assert g.max() > 0.6 and ((g > 0) & (g < 2.0 ** -100) & ~exact_zero).sum() > 5   # tiny gates that are NOT zero
        # the derived floor grows with the opacity
        rel = bound.min(1) / np.abs(want).max(1)
        live = ~exact_zero & (np.abs(want).max(1) > 1e-30)          # below that the absolute floor 2^-126 governs
        assert live.sum() > 100
        assert rel[live][-1] > 2.5 * rel[live][0] and rel[live].max() < 1e-4
    # rows of a shard draw the whole set's normals
    np.testing.assert_array_equal(mc.normals_at(np.arange(N), 9, 5), mo.normals(N, 9, 5))
    if N > 3:
        sh = mc.noise_f32(P["quats"][3:], P["scales"][3:], P["opacities"][3:], 500.0, 9, 5, row_offset=3)
        np.testing.assert_array_equal(sh, mc.noise_f32(P["quats"], P["scales"], P["opacities"], 500.0, 9, 5)[3:])
