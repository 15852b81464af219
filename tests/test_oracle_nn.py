"""Pins oracle/nn_oracle.py (path A restatement, "parity unpinned vs upstream") -- CPU only."""
import numpy as np
import pytest

import nn_cases as nc
from oracle import nn_oracle as no


def test_nn_dot_is_bruteforce_argmax():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((50, 24)).astype(np.float32); d = rng.standard_normal((3000, 24)).astype(np.float32)
    idx, best, second = no.nn_dot(q, d, block=512, dtype=np.float64)
    s = q.astype(np.float64) @ d.astype(np.float64).T
    assert np.array_equal(idx, s.argmax(1))
    np.testing.assert_allclose(best, s.max(1))
    np.testing.assert_allclose(second, np.sort(s, 1)[:, -2])


def test_first_index_wins_ties():
    d = np.zeros((10, 24), np.float32); d[3, 0] = 1; d[7, 0] = 1
    q = np.zeros((1, 24), np.float32); q[0, 0] = 2
    assert no.nn_dot(q, d, block=4)[0][0] == 3


def test_reciprocal_matches_are_mutual_and_recover_planted_pairs():
    H, W = 48, 64
    A, B, src, dst = no.synth_descriptors(H, W, planted=0.2, seed=1)
    xy1, xy2 = no.fast_reciprocal_NNs(A, B, S=4)
    Af, Bf = A.reshape(-1, 24).astype(np.float64), B.reshape(-1, 24).astype(np.float64)
    # every returned pair is a mutual nearest neighbour
    assert np.array_equal((Af[xy1] @ Bf.T).argmax(1), xy2)
    assert np.array_equal((Bf[xy2] @ Af.T).argmax(1), xy1)
    # sorted, unique
    key = xy2.astype(np.int64) | (xy1.astype(np.int64) << 32)
    assert np.all(np.diff(key) > 0)
    planted = dict(zip(src.tolist(), dst.tolist()))
    hits = sum(1 for a, b in zip(xy1.tolist(), xy2.tolist()) if planted.get(a) == b)
    assert hits > 0.25 * len(xy1) and hits >= 20  # random descriptors also produce some mutual pairs


# ---- the shapes and inputs of tests/test_gpu_nn.py (tests/nn_cases.py) ----

def test_case_list_reaches_every_path_of_the_argmax_kernel():
    """st3r_nn_plan on every case: the list as a whole still holds each path of k_nn_argmax / wave_resolve it was written
    for.  A retuned heuristic that moves a shape off its path fails here instead of thinning the GPU tests silently."""
    full_counts, S_seen, ragged_alone = set(), set(), False
    for n, m in nc.CASES:
        S, tps = nc.plan(n, m)
        tiles = (m + 31) // 32
        assert S >= 1 and tps >= 1 and (S - 1) * tps < tiles <= S * tps, (n, m, S, tps)   # every tile once, no empty segment
        segs = nc.segments(m, S, tps)
        assert sum(f + r for f, r in segs) == tiles
        full_counts |= {f for f, _ in segs}
        S_seen.add(S)
        ragged_alone |= segs[-1] == (0, True) and S > 1
    assert {0, 1, 2, 3, 4, 5} <= full_counts and max(full_counts) >= 7, sorted(full_counts)
    assert 1 in S_seen and any(2 * S > 64 for S in S_seen), sorted(S_seen)
    assert ragged_alone
    ms = {m for _, m in nc.CASES}; ns = {n for n, _ in nc.CASES}
    assert {0, 1, 31} <= {m % 32 for m in ms}
    assert {1, 3, 4, 5, 31, 32, 33} <= ms
    assert {1, 31, 32, 33, 63, 64, 65, 129} <= ns
    # the families run on the list or on stated parts of it
    assert set(nc.UNNORMALISED) <= set(nc.CASES) and set(nc.LARGE) <= set(nc.CASES) and set(nc.LARGE) <= set(nc.SELF_MATCH)
    assert {m for _, m in nc.ALL_NEGATIVE} == {m for m in ms if m % 32} and {1, 3, 4, 5, 31} <= {m for _, m in nc.ALL_NEGATIVE}
    # the duplicated rows that must tie across the ballot chunks of wave_resolve do have more than 64 partials
    n, m0, r = nc.DUPLICATED[-1]
    assert n <= 64 and 2 * nc.plan(n, m0 * r)[0] > 64


def test_nn_plan_rejects_nonsense():
    import ctypes as C
    from starst3r_amd import _lib
    S, tps = C.c_int(0), C.c_int(0)
    L = _lib.lib()
    assert L.st3r_nn_plan(0, 5, C.byref(S), C.byref(tps)) != 0 and L.st3r_nn_plan(5, 0, C.byref(S), C.byref(tps)) != 0
    assert L.st3r_nn_plan(5, 5, None, C.byref(tps)) != 0


@pytest.mark.parametrize("family", sorted(nc.FAMILIES))
def test_every_gpu_argmax_input_is_all_clear(family):
    """No query of any (builder, shape) pair the GPU tests use is a numerical tie, so they may compare every query; and
    the builders do what their names say."""
    for args in nc.FAMILIES[family]:
        q, d, idx, best, clear = nc.reference(family, args)
        assert q.shape == (args[0], nc.D) and q.dtype == np.float32 and d.dtype == np.float32
        assert clear.all(), (family, args, int((~clear).sum()))
        if family == "self":
            assert d.shape[0] == args[1] and np.array_equal(idx, np.arange(args[0]) % args[1])
        elif family == "neg":
            assert best.max() < 0
        elif family == "unnorm":
            nrm = np.linalg.norm(d.astype(np.float64), axis=1)
            assert (best > 0).all() or args[1] < 8      # mixed sign: with a handful of rows the best may be negative
            assert args[1] < 100 or nrm.max() / nrm.min() > 100
        elif family == "dup":
            n, m0, r = args
            assert d.shape[0] == m0 * r and all(np.array_equal(d[:m0], d[k * m0:(k + 1) * m0]) for k in range(r))
            assert idx.max() < m0
        elif family == "planted":
            assert (idx == args[2]).all()


def test_seed_count_is_numpys_grid():
    from starst3r_amd import _lib
    L = _lib.lib()
    for S in range(1, 21):
        for H in range(1, 41):
            ny = len(range(S // 2, H, S))
            for W in range(1, 41):
                assert L.st3r_recip_nn_seed_count(H, W, S) == ny * len(range(S // 2, W, S)), (H, W, S)
    assert np.mgrid[3:25:7, 3:41:7].reshape(2, -1).shape[1] == L.st3r_recip_nn_seed_count(25, 41, 7)
    assert L.st3r_recip_nn_seed_count(0, 5, 2) == 0 and L.st3r_recip_nn_seed_count(5, 5, 0) == 0


@pytest.mark.parametrize("name", sorted(nc.LOOP_CASES))
def test_loop_state_merges_to_the_plain_result_and_is_all_clear(name):
    """return_state=True is the same loop (its converged state merges to the plain return value); no seed of a GPU
    loop case meets an unclear query at any max_iter, so the GPU test compares every seed; the convergence counts are the
    ones the cases were chosen for (both notyet values after 1 and 2 iterations, all converged after 10)."""
    A, B, S = nc.loop_scene(name)
    from starst3r_amd import _lib
    seeds = _lib.lib().st3r_recip_nn_seed_count(A.shape[0], A.shape[1], S)
    for k, it in enumerate(nc.LOOP_ITERS):
        xy1, xy2, notyet, unclear = nc.loop_reference(name, it)
        assert len(xy1) == len(xy2) == len(notyet) == len(unclear) == seeds == nc.LOOP_CONVERGED[name][3]
        m1, m2 = no.fast_reciprocal_NNs(A, B, S=S, max_iter=it, dtype=np.float64)
        e1, e2 = no.merge_corres(xy1[~notyet], xy2[~notyet])
        assert np.array_equal(m1, e1) and np.array_equal(m2, e2)
        assert not unclear.any(), (name, it, int(unclear.sum()))
        assert int((~notyet).sum()) == nc.LOOP_CONVERGED[name][k]
        assert xy2.min() >= 0 and xy2.max() < B.shape[0] * B.shape[1] and xy1.max() < A.shape[0] * A.shape[1]
    seeds_by_name = {n: nc.LOOP_CONVERGED[n][3] for n in nc.LOOP_CASES}
    assert seeds_by_name["1536_seeds"] > 1024 and seeds_by_name["1024_seeds"] == 1024 and seeds_by_name["1025_seeds"] == 1025
    # the mixed sizes do plan differently for the two directions
    for n in ("cropped_B", "two_scenes"):
        a, b, _ = nc.loop_scene(n)
        k = seeds_by_name[n]
        assert nc.plan(k, a.shape[0] * a.shape[1])[0] != nc.plan(k, b.shape[0] * b.shape[1])[0]


def test_older_loop_scenes_are_all_clear():
    """test_fast_reciprocal_nns_vs_oracle asks for set equality on these scenes: the float64 trajectory of every seed
    is clear of numerical ties."""
    for (H, W), S in nc.VS_ORACLE:
        A, B, _, _ = no.synth_descriptors(H, W, planted=0.2, seed=3)
        assert not no.fast_reciprocal_NNs(A, B, S=S, dtype=np.float64, return_state=True)[3].any()


def test_clear_rule_scales_with_the_rows():
    """Unit rows: the 1e-5 relative term decides.  Rows of length 100: the float32 error term does."""
    q = np.zeros((1, 24), np.float32); q[0, 0] = 1
    d = np.zeros((2, 24), np.float32); d[:, 0] = 1
    assert no.clear_queries(q, d, np.array([1.0]), np.array([1.0 - 2e-5]))[0]
    assert not no.clear_queries(q, d, np.array([1.0]), np.array([1.0 - 5e-6]))[0]
    assert not no.clear_queries(q, 100 * d, np.array([1.0]), np.array([1.0 - 2e-5]))[0]
    assert no.clear_queries(q, 100 * d, np.array([1.0]), np.array([1.0 - 3e-4]))[0]
