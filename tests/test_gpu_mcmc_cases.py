"""GPU side of tests/mcmc_cases.py: csrc/mcmc.hip + csrc/scan.h through `ops`, one call per case, nothing masked.
Integer state (prefix sums, ranks, draws, counts) is compared for equality with numpy evaluated WITHOUT the device's
prefix sums; relocated values within mcmc_cases.reloc_bound, noise within mcmc_cases.noise_bound (derivations there)."""
import numpy as np
import pytest
import torch

import mcmc_cases as mc
from oracle import mcmc_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    return ops.get_context(torch.device(DEV))


def to_dev(P, extra=0, fill=float("nan")):
    return {k: torch.cat([torch.from_numpy(v), torch.full((extra,) + v.shape[1:], fill)]).to(DEV) if extra
            else torch.from_numpy(v.copy()).to(DEV) for k, v in P.items()}


def to_np(D):
    return {k: v.cpu().numpy() for k, v in D.items()}


def relocate(ctx, P, min_opacity, seed, step, m=None, v=None):
    """One call; returns (got, n_dead, cum, dead, sampled, dead_ids, count)."""
    from starst3r_amd import ops
    N = P["means"].shape[0]
    D = to_dev(P)
    n = ops.mcmc_relocate(ctx, D, m, v, min_opacity, seed=seed, step=step)
    cum = ops.peek(ctx, 4, N, torch.int64).cpu().numpy().view(np.uint64)
    dead = ops.peek(ctx, 5, N, torch.int32).cpu().numpy()
    st = ops.peek(ctx, 6, 2 * N, torch.int32).cpu().numpy()
    count = ops.peek(ctx, 7, N, torch.int32).cpu().numpy()
    return to_np(D), n, cum, dead, st[:n].astype(np.int64), st[N:N + n].astype(np.int64), count


def add(ctx, P, n_new, min_opacity, seed, step):
    from starst3r_amd import ops
    N = P["means"].shape[0]
    D = to_dev(P, n_new)
    ops.mcmc_add(ctx, D, N, n_new, min_opacity, seed=seed, step=step)
    cum = ops.peek(ctx, 4, N, torch.int64).cpu().numpy().view(np.uint64)
    sampled = ops.peek(ctx, 6, n_new, torch.int32).cpu().numpy().astype(np.int64)
    count = ops.peek(ctx, 7, N, torch.int32).cpu().numpy()
    return to_np(D), cum, sampled, count


# ------------------------------------------------------------------------------------------------- 1. exact weights
@pytest.mark.parametrize("N", mc.EXACT_N)
def test_exact_weights_scan_ranks_draws(ctx, N):
    c = mc.exact_case(N)
    P, w = c["P"], c["w"]
    cum_ref = np.cumsum(w, dtype=np.uint64)
    dead_ref = w == 0
    # relocate: 64-bit inclusive scan, 32-bit exclusive rank scan, draws over the alive
    got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, c["min_opacity"], c["seed"], c["step"])
    np.testing.assert_array_equal(cum, cum_ref)
    np.testing.assert_array_equal(dead.astype(bool), dead_ref)
    assert n == int(dead_ref.sum())
    np.testing.assert_array_equal(dead_ids, np.nonzero(dead_ref)[0])
    Q = {k: v.copy() for k, v in P.items()}
    ids_o, sampled_o = mo.relocate(Q, None, c["min_opacity"], seed=c["seed"], step=c["step"])
    np.testing.assert_array_equal(ids_o, dead_ids)
    np.testing.assert_array_equal(sampled, sampled_o)
    np.testing.assert_array_equal(count, np.bincount(sampled_o, minlength=N) if len(sampled_o) else np.zeros(N, int))
    assert not dead_ref[sampled].any()
    worst = mc.check_relocated(P, got, sampled, dead_ids, c["min_opacity"])
    # grow: the same prefix sums (nobody is dead, the zeros weigh nothing), stream 1
    got, cum, sampled, count = add(ctx, P, c["n_new"], c["min_opacity"], c["seed"], c["step"])
    np.testing.assert_array_equal(cum, cum_ref)
    Q = {k: v.copy() for k, v in P.items()}
    _, sampled_o = mo.add_new(Q, c["n_new"], c["min_opacity"], seed=c["seed"], step=c["step"])
    np.testing.assert_array_equal(sampled, sampled_o)
    np.testing.assert_array_equal(count, np.bincount(sampled_o, minlength=N))
    assert not dead_ref[sampled].any()
    worst = max(worst, mc.check_relocated(P, got, sampled, N + np.arange(c["n_new"]), c["min_opacity"]))
    print("exact N=%d relocation worst error / bound %.3f" % (N, worst))


# ------------------------------------------------------------------------------------------------- 2. plateaus
def test_sampler_plateaus_4096_draws(ctx):
    lg = mc.plateau_logits()
    P = mc.params(64, lg, seed=2)
    w = mc.exact_weights(lg)
    got, cum, sampled, count = add(ctx, P, 4096, 0.005, seed=(9 << 32) | 5, step=3)
    np.testing.assert_array_equal(cum, np.cumsum(w, dtype=np.uint64))
    want = mo.draw(np.cumsum(w, dtype=np.uint64), np.arange(4096), mo.STREAM_ADD, 3, (9 << 32) | 5)
    np.testing.assert_array_equal(sampled, want)
    assert (w[sampled] > 0).all()
    np.testing.assert_array_equal(count, np.bincount(want, minlength=64))


def test_sampler_draws_that_equal_a_prefix_sum(ctx):
    lg = mc.tiny_logits()
    P = mc.params(64, lg, seed=4)
    w, _ = mo.weights(lg, 0.005, False)
    got, cum, sampled, count = add(ctx, P, 2048, 0.005, seed=6, step=2)
    np.testing.assert_array_equal(cum, np.cumsum(w, dtype=np.uint64))
    want = mo.draw(np.cumsum(w, dtype=np.uint64), np.arange(2048), mo.STREAM_ADD, 2, 6)
    np.testing.assert_array_equal(sampled, want)
    assert (w[sampled] > 0).all()


def test_add_with_every_weight_zero_takes_the_last_row(ctx):
    """All logits -200: total weight 0, every draw falls off the end of the search and is clamped to N - 1 (kernel and
    oracle alike).  The source's sigmoid is 0: new opacity 0 -> clamped to min_opacity, scale factor 0 / 0 -> NaN scales
    (DESIGN.md records it)."""
    P = mc.params(64, np.full(64, mc.L_ZERO), seed=3)
    got, cum, sampled, count = add(ctx, P, 5, 0.005, seed=1, step=1)
    assert (cum == 0).all() and (sampled == 63).all() and count[63] == 5 and count[:63].sum() == 0
    Q = {k: v.copy() for k, v in P.items()}
    with np.errstate(all="ignore"):
        grown, sampled_o = mo.add_new(Q, 5, 0.005, seed=1, step=1)
    assert (sampled_o == 63).all()
    assert np.isnan(got["scales"][63]).all() and np.isnan(grown["scales"][63]).all()
    assert abs(float(got["opacities"][63]) - float(grown["opacities"][63])) <= 4 * 2.0 ** -23 * abs(float(grown["opacities"][63]))
    for k in P:
        np.testing.assert_array_equal(got[k][:63].view(np.uint32), P[k][:63].view(np.uint32))
        np.testing.assert_array_equal(got[k][64:].view(np.uint32), np.broadcast_to(got[k][63], got[k][64:].shape).view(np.uint32))


# ------------------------------------------------------------------------------------------------- 3. ratio clamp
def test_ratio_clamp_at_51(ctx):
    res = {}
    for n_dead in (48, 49, 50, 51, 69):
        P = mc.single_source(F(0.3), n_dead)
        got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.005, seed=4, step=2)
        assert n == n_dead and (sampled == 0).all() and count[0] == n_dead
        mc.check_relocated(P, got, sampled, dead_ids, 0.005)
        res[n_dead] = (got["opacities"][0].tobytes(), got["scales"][0].tobytes())
    assert res[50] == res[51] == res[69]                    # count + 1 = 51, 52, 70 -> n_idx 51
    assert len({res[48], res[49], res[50]}) == 3            # 49, 50, 51 differ


def test_two_sources_with_different_counts_in_one_call(ctx):
    P = mc.two_sources()
    got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.005, seed=11, step=0)
    Q = {k: v.copy() for k, v in P.items()}
    _, sampled_o = mo.relocate(Q, None, 0.005, seed=11, step=0)
    np.testing.assert_array_equal(sampled, sampled_o)
    assert n == 60 and count[7] + count[40] == 60 and 0 < count[40] < count[7] and count[7] + 1 > 51
    mc.check_relocated(P, got, sampled, dead_ids, 0.005)


# ------------------------------------------------------------------------------------------------- 4. accuracy
@pytest.mark.parametrize("ratio", mc.GRID_RATIO)
def test_relocation_accuracy_grid(ctx, ratio):
    for o in mc.GRID_O:
        P = mc.single_source(mc.logit_of(o), ratio - 1)
        got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.005, seed=8, step=1)
        assert count[0] == ratio - 1
        b = mc.reloc_bound(P["opacities"][0], P["scales"][0], ratio, 0.005)
        assert b["in_domain"]
        e_lg = abs(float(got["opacities"][0]) - b["ref_logit"])
        e_ls = float(np.abs(got["scales"][0].astype(np.float64) - b["ref_logscale"]).max())
        print("o=%.8g ratio=%d  logit err %.2e / bound %.2e (oracle %.2e)   log-scale err %.2e / bound %.2e (oracle %.2e)"
              % (o, ratio, e_lg, b["bound_logit"], b["yard_logit"], e_ls, b["bound_logscale"], b["yard_logscale"]))
        mc.check_relocated(P, got, sampled, dead_ids, 0.005)


@pytest.mark.parametrize("logit,count", [(20.0, 24), (20.0, 31), (20.0, 39), (17.0, 39), (20.0, 45), (20.0, 46), (20.0, 48),
                                         (20.0, 49), (20.0, 50), (20.0, 69)])
def test_outside_the_float32_domain_kernel_and_oracle_agree_in_sign_and_finiteness(ctx, logit, count):
    """o == 1.0f and ratio >= 25: the alternating binomial sum has lost every digit, from ratio 32 on it is negative
    (upstream's arithmetic, kept).  Counts 31, 46, 48, 49 are ratios at which a fused multiply-add in the sum gives the
    other sign than the separately rounded reference."""
    P = mc.single_source(F(logit), count)
    b = mc.reloc_bound(P["opacities"][0], P["scales"][0], count + 1, 0.005)
    assert not b["in_domain"]
    got, n, cum, dead, sampled, dead_ids, cnt = relocate(ctx, P, 0.005, seed=8, step=1)
    assert cnt[0] == count
    mc.check_relocated(P, got, sampled, dead_ids, 0.005)     # logit within its bound; scales: sign and finiteness


# ------------------------------------------------------------------------------------------------- 5. thresholds
def test_dead_threshold_is_inclusive(ctx):
    P = mc.params(4, np.array([0.0, 1e-3, 3.0, -1e-3], F), seed=6)
    got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.5, seed=2, step=2)
    assert dead.tolist() == [1, 0, 0, 1] and n == 2 and dead_ids.tolist() == [0, 3]
    w, _ = mo.weights(P["opacities"], 0.5, True)
    np.testing.assert_array_equal(cum, np.cumsum(w, dtype=np.uint64))
    mc.check_relocated(P, got, sampled, dead_ids, 0.5)


def test_opacity_clamps(ctx):
    # barely above min_opacity, ratio 3: the new opacity is far below it -> the lower clamp
    P = mc.single_source(F(1e-3), 2)
    got, n, *_rest = relocate(ctx, P, 0.5, seed=1, step=1)
    b = mc.reloc_bound(P["opacities"][0], P["scales"][0], 3, 0.5)
    assert n == 2 and b["ref_logit"] == 0.0 and abs(float(got["opacities"][0])) <= b["bound_logit"] <= 1e-6
    # logit 20 (sigmoid exactly 1), ratio 2: new opacity 1 -> the upper clamp 1 - eps, logit log(2^23 - 1)
    P = mc.single_source(F(20.0), 1)
    got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.005, seed=1, step=1)
    b = mc.reloc_bound(P["opacities"][0], P["scales"][0], 2, 0.005)
    assert abs(b["ref_logit"] - np.log(2.0 ** 23 - 1)) < 1e-12
    assert abs(float(got["opacities"][0]) - b["ref_logit"]) <= b["bound_logit"] <= 4e-6
    mc.check_relocated(P, got, sampled, dead_ids, 0.005)


@pytest.mark.parametrize("shN_rows,with_sh0,with_adam", [(4, True, True), (24, True, True), (24, False, False),
                                                         (4, False, True), (24, True, False)])
def test_adam_zeroing_and_sh_layouts(ctx, shN_rows, with_sh0, with_adam):
    """m, v hold a distinct non-zero value per float: exactly the 23 floats of every source row become 0 (the shN
    block is 12 wide even when a parameter row has 72 floats), nobody else's change.  NaN in the unused SH tail rides
    along bit for bit; sh0 may be absent."""
    N = 300
    rng = np.random.default_rng(shN_rows)
    lg = rng.uniform(-2, 2, N).astype(F); lg[rng.choice(N, 40, replace=False)] = -9.0
    P = mc.params(N, lg, shN_rows=shN_rows, sh0=with_sh0, seed=9)
    if shN_rows > 4:
        P["shN"][::3, 4:] = np.nan
        P["shN"][5, 23, 2] = np.inf
    # [23N] moments followed by a guard of 61N floats (a 72-wide shN block would end at 83N): nothing behind the
    # buffer may change either
    m0 = np.arange(1, 84 * N + 1, dtype=F); v0 = -m0
    m_all = torch.from_numpy(m0.copy()).to(DEV); v_all = torch.from_numpy(v0.copy()).to(DEV)
    m = m_all[:23 * N] if with_adam else None
    v = v_all[:23 * N] if with_adam else None
    got, n, cum, dead, sampled, dead_ids, count = relocate(ctx, P, 0.005, seed=77, step=4, m=m, v=v)
    Q = {k: x.copy() for k, x in P.items()}
    _, sampled_o = mo.relocate(Q, None, 0.005, seed=77, step=4)
    assert n == 40
    np.testing.assert_array_equal(sampled, sampled_o)
    mc.check_relocated(P, got, sampled, dead_ids, 0.005)
    if with_adam:
        src = np.unique(sampled)
        for buf, ref in ((m_all, m0), (v_all, v0)):
            want = ref.copy(); off = 0
            for width in (3, 4, 3, 1, 12):
                blk = want[off * N:(off + width) * N].reshape(N, width); blk[src] = 0; off += width
            np.testing.assert_array_equal(buf.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------- 6. noise
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("step,seed", [(0, 5), (9, (0xDEADBEEF << 32) | 5)])
def test_noise_on_zero_means(ctx, N, step, seed):
    from starst3r_amd import ops
    P = mc.noise_case(N)
    scaler = 1e-3 * 5e5
    D = to_dev(P)
    ops.mcmc_noise(ctx, D, scaler, seed=seed, step=step)
    got = D["means"].cpu().numpy().astype(np.float64)
    want, bound, yard, exact_zero = mc.noise_bound(P, scaler, step, seed)
    err = np.abs(got - want)
    print("noise N=%d worst error / bound %.3f (float32 restatement: %.3f)" % (N, (err / bound).max(), (yard / bound).max()))
    assert (err <= bound).all(), (np.argmax(err / bound), (err / bound).max())
    assert (got[exact_zero] == 0).all()
    for k in ("quats", "scales", "opacities", "shN", "sh0"):
        np.testing.assert_array_equal(D[k].cpu().numpy().view(np.uint32), P[k].view(np.uint32))


def test_noise_of_a_shard_equals_the_whole_sets_rows(ctx):
    from starst3r_amd import ops
    P = mc.noise_case(257 + 256)
    whole = to_dev(P)
    ops.mcmc_noise(ctx, whole, 500.0, seed=(3 << 32) | 1, step=6)
    whole = whole["means"].cpu().numpy()
    for lo in (1, 255, 256):
        for n in (1, 257):
            S = to_dev({k: v[lo:lo + n] for k, v in P.items()})
            ops.mcmc_noise(ctx, S, 500.0, seed=(3 << 32) | 1, step=6, row_offset=lo)
            np.testing.assert_array_equal(S["means"].cpu().numpy().view(np.uint32), whole[lo:lo + n].view(np.uint32))
    assert (whole[1:258] != whole[0:257]).any()
