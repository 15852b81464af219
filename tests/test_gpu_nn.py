"""GPU parity tests for path A: MFMA dot-product arg-max and the reciprocal-NN loop vs oracle/nn_oracle.py.

Indices must be exact wherever the decision is not a numerical tie: the HIP kernel accumulates the 24
products in fp32 in its own order (exact fp32 MFMA), the reference uses a BLAS matmul in fp32 with an
unspecified order, so a query whose best and runner-up float64 scores differ by less than 1e-5 (relative)
may legitimately pick either; such queries are counted and must be rare.

The shapes and inputs of tests/nn_cases.py go further: they are built so that NO query is a numerical tie (asserted on
the CPU by tests/test_oracle_nn.py, together with the kernel paths the shapes reach), so every query and every seed of
the reciprocal loop is compared, and the score is held to the worst-case error of a 24-term float32 dot product."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nn_cases as nc
from oracle import nn_oracle as no


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    return ops.get_context("cuda:0")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


@pytest.mark.parametrize("n,m", [(1, 33), (64, 32), (100, 1000), (3072, 196608), (777, 50001)])
def test_argmax_vs_float64_bruteforce(ctx, n, m):
    from starst3r_amd import matching
    rng = np.random.default_rng(n + m)
    q = rng.standard_normal((n, 24)).astype(np.float32); d = rng.standard_normal((m, 24)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True); d /= np.linalg.norm(d, axis=1, keepdims=True)
    nn, score = matching.nn_dot_argmax(ctx, dev(q), dev(d), want_score=True)
    torch.cuda.synchronize()
    nn = nn.cpu().numpy(); score = score.cpu().numpy()
    idx, best, second = no.nn_dot(q, d, dtype=np.float64)
    clear = (best - second) > 1e-5 * np.abs(best)
    assert clear.mean() > 0.99
    assert np.array_equal(nn[clear], idx[clear])
    # a near-tie may pick the runner-up, never anything worse
    s_pick = np.einsum("ij,ij->i", q.astype(np.float64), d[nn].astype(np.float64))
    assert np.all(s_pick >= second - 1e-5 * np.abs(best))
    np.testing.assert_allclose(score, s_pick, rtol=1e-5, atol=1e-6)


def test_exact_ties_pick_first_index(ctx):
    from starst3r_amd import matching
    d = np.zeros((500, 24), np.float32); d[[77, 300, 499], 5] = 1.0
    q = np.zeros((3, 24), np.float32); q[:, 5] = 1.0
    nn = matching.nn_dot_argmax(ctx, dev(q), dev(d)).cpu().numpy()
    assert nn.tolist() == [77, 77, 77]


@pytest.mark.parametrize("shape,S", [((48, 64), 4), ((96, 128), 8)])
def test_fast_reciprocal_nns_vs_oracle(ctx, shape, S):
    from starst3r_amd import matching
    H, W = shape
    A, B, src, dst = no.synth_descriptors(H, W, planted=0.2, seed=3)
    i1, i2 = matching.fast_reciprocal_NNs(dev(A), dev(B), subsample_or_initxy1=S, ret_xy=False, device="cuda:0")
    torch.cuda.synchronize()
    i1 = i1.cpu().numpy(); i2 = i2.cpu().numpy()
    o1, o2 = no.fast_reciprocal_NNs(A, B, S=S, dtype=np.float64)
    got = set(zip(i1.tolist(), i2.tolist())); exp = set(zip(o1.tolist(), o2.tolist()))
    # both scenes are clear of near ties along the whole float64 trajectory of every seed (nn_cases.VS_ORACLE, pinned by
    # test_oracle_nn.py::test_older_loop_scenes_are_all_clear), so the sets are equal; the former 1 % allowance for
    # near-tie flips is needed by neither
    assert (shape, S) in nc.VS_ORACLE
    assert got == exp, (len(got), len(exp), sorted(got ^ exp)[:8])
    assert np.array_equal(i1, o1) and np.array_equal(i2, o2)
    # output contract of merge_corres: unique, sorted on (idx2, idx1)
    key = i2.astype(np.int64) | (i1.astype(np.int64) << 32)
    assert np.all(np.diff(key) > 0)
    xy1, xy2 = matching.fast_reciprocal_NNs(dev(A), dev(B), subsample_or_initxy1=S, ret_xy=True, device="cuda:0")
    assert np.array_equal(xy1.cpu().numpy()[:, 0] + W * xy1.cpu().numpy()[:, 1], i1)


def stepwise_equals_device_loop(ctx, A, B, S):
    from starst3r_amd import matching
    H, W = A.shape[:2]
    Ad = dev(A).reshape(-1, A.shape[-1]).contiguous(); Bd = dev(B).reshape(-1, B.shape[-1]).contiguous()
    y1, x1 = np.mgrid[S // 2:H:S, S // 2:W:S].reshape(2, -1)
    xy1 = torch.as_tensor(np.int32(np.unique(x1 + W * y1)), device="cuda:0")
    xy2 = torch.full_like(xy1, -1); old1 = xy1.clone(); old2 = xy2.clone()
    notyet = torch.ones_like(xy1, dtype=torch.bool)
    for it in range(10):
        if not bool(notyet.any()):
            break
        act = torch.nonzero(notyet).reshape(-1)
        xy2[act] = matching.nn_dot_argmax(ctx, Ad[xy1[act].long()], Bd)
        notyet &= (old2 != xy2)
        act = torch.nonzero(notyet).reshape(-1)
        xy1[act] = matching.nn_dot_argmax(ctx, Bd[xy2[act].long()], Ad)
        notyet &= (old1 != xy1)
        old2.copy_(xy2); old1.copy_(xy1)
    conv = ~notyet
    e1, e2 = matching.merge_corres(xy1[conv], xy2[conv], ret_xy=False)
    g1, g2 = matching.fast_reciprocal_NNs(dev(A), dev(B), subsample_or_initxy1=S, ret_xy=False, device="cuda:0")
    assert g1.numel() > 0 and torch.equal(g1, e1) and torch.equal(g2, e2)


@pytest.mark.parametrize("shape,S", [((48, 64), 4), ((96, 128), 8), ((50, 70), 8)])
def test_device_resident_loop_equals_stepwise_loop(ctx, shape, S):
    """st3r_recip_nn (no host round trip) == the same iteration driven step by step from the host with
    st3r_nn_dot_argmax: identical arithmetic, so identical indices and convergence flags."""
    H, W = shape
    A, B, _, _ = no.synth_descriptors(H, W, planted=0.3, seed=11)
    stepwise_equals_device_loop(ctx, A, B, S)


@pytest.mark.parametrize("name", ["1536_seeds", "cropped_B", "two_scenes"])
def test_device_resident_loop_equals_stepwise_loop_chunks_and_mixed_sizes(ctx, name):
    """The same with more seeds than one chunk of k_nn_compact, and with maps of different sizes (two plans, partial
    buffers laid out by the larger one)."""
    stepwise_equals_device_loop(ctx, *nc.loop_scene(name))


# ---- every tile, segment, tie and loop edge (tests/nn_cases.py) ----

worst_score_ratio = [0.0]


def argmax_parity(ctx, family, args):
    """Exact indices for every query and |score - float64| <= 24 * 2^-24 * sum |q_k d_k| of the chosen row."""
    from starst3r_amd import matching
    q, d, idx, best, clear = nc.reference(family, args)
    assert clear.all()
    nn, score = matching.nn_dot_argmax(ctx, dev(q), dev(d), want_score=True)
    torch.cuda.synchronize()
    nn = nn.cpu().numpy(); score = score.cpu().numpy().astype(np.float64)
    bad = np.nonzero(nn != idx)[0]
    assert bad.size == 0, (family, args, bad.size, bad[:8].tolist(), nn[bad[:8]].tolist(), idx[bad[:8]].tolist())
    bound = nc.score_bound(q, d, idx)
    ratio = float((np.abs(score - best) / bound).max())
    worst_score_ratio[0] = max(worst_score_ratio[0], ratio)
    print(f"{family} {args}: worst |score - float64| / bound = {ratio:.3f} (so far {worst_score_ratio[0]:.3f})")
    assert ratio <= 1.0, (family, args, ratio)


@pytest.mark.parametrize("n,m", nc.SELF_MATCH)
def test_argmax_self_match(ctx, n, m):
    """Query i is row i % m of random unit rows: every row of every tile, half-wave, segment and ragged position has to
    win once (float64 gap to the runner-up >= 0.13 at 4231 rows)."""
    argmax_parity(ctx, "self", (n, m))


@pytest.mark.parametrize("n,m", nc.ALL_NEGATIVE)
def test_argmax_all_negative_scores(ctx, n, m):
    """Every score is negative and m is no multiple of 32: the zero-padded rows of the ragged tile score exactly 0 and win
    unless both `rr < m` masks hold; m < 4 leaves half-wave 1 without a valid row."""
    argmax_parity(ctx, "neg", (n, m))


@pytest.mark.parametrize("n,m", nc.UNNORMALISED)
def test_argmax_unnormalised_mixed_sign(ctx, n, m):
    """Rows and queries of lengths 0.05 .. 500: the clear-query rule with the float32 error term, and the score bound,
    on inputs that are not unit descriptors."""
    argmax_parity(ctx, "unnorm", (n, m))


@pytest.mark.parametrize("n,m0,r", nc.DUPLICATED)
def test_argmax_duplicated_rows_pick_the_first_copy(ctx, n, m0, r):
    """Exact ties inside one partial, across the half-waves of a tile, across tiles, in the ragged tile, across
    segments and across the ballot chunks of wave_resolve, for query tiles 0 and 1 and a second query group: the answer
    is the float64 arg-max over the distinct rows, which is the smallest tied index."""
    argmax_parity(ctx, "dup", (n, m0, r))


@pytest.mark.parametrize("n,m,row", nc.PLANTED)
def test_argmax_answer_in_first_and_last_row(ctx, n, m, row):
    argmax_parity(ctx, "planted", (n, m, row))


def recip_nn_state(ctx, A, B, S, max_iter):
    """st3r_recip_nn through the C ABI, as matching.fast_reciprocal_NNs calls it -> (idx1, idx2, notyet) per seed."""
    from starst3r_amd import _lib, ops
    H1, W1, D = A.shape; H2, W2, _ = B.shape
    Ad = dev(A).reshape(-1, D).contiguous(); Bd = dev(B).reshape(-1, D).contiguous()
    lib = _lib.lib()
    n = lib.st3r_recip_nn_seed_count(H1, W1, S)
    out = [torch.full((n,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    _lib.check(lib.st3r_recip_nn(ctx.handle, ops._stream(), ops._p(Ad), H1, W1, ops._p(Bd), H2, W2, D, S, max_iter,
                                 *(ops._p(t, torch.int32) for t in out)))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("max_iter", nc.LOOP_ITERS)
@pytest.mark.parametrize("name", sorted(nc.LOOP_CASES))
def test_reciprocal_loop_state_vs_oracle_seed_by_seed(ctx, name, max_iter):
    """idx1, idx2 and notyet of EVERY seed against the float64 oracle's loop state (no seed of these scenes meets a
    numerical tie), after 1 and 2 iterations -- converged and moving seeds side by side -- and after 10: more seeds than
    one chunk of k_nn_compact, exactly one chunk, one chunk and one seed, and maps of different sizes."""
    A, B, S = nc.loop_scene(name)
    xy1, xy2, notyet, unclear = nc.loop_reference(name, max_iter)
    assert not unclear.any()
    g1, g2, gn = recip_nn_state(ctx, A, B, S, max_iter)
    assert len(g1) == len(xy1)
    assert set(np.unique(gn).tolist()) <= {0, 1}
    assert np.array_equal(gn != 0, notyet), (int((gn != 0).sum()), int(notyet.sum()), np.nonzero((gn != 0) != notyet)[0][:8])
    assert np.array_equal(g2, xy2), np.nonzero(g2 != xy2)[0][:8]
    assert np.array_equal(g1, xy1), np.nonzero(g1 != xy1)[0][:8]
