"""GPU parity tests of the fused Adam step (csrc/adam.hip) through the C ABI, on every launch shape st3r_adam_impl
distinguishes: the scalar kernel k_adam (N % 4 != 0, or any buffer not 16-byte aligned), the four-wide k_adam4 (N % 4 == 0
and everything aligned), the grid-stride loop of either (more than 4096 blocks of 256 threads' worth of work), first and
late steps, cold and warm state, zero gradients on zero state.  Oracle and bounds are test_adam_vs_oracle_and_torch's:
oracle/gs_oracle.c gso_adam (torch.optim.Adam's single-tensor arithmetic), parameters atol 3e-7, moments rtol 1e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_adam_cases as lac
from st3r_synth import synth


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context("cuda:0")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def gaussians(N, seed):
    g = synth.make_gaussians(N, seed=seed)
    # SH rows 4..23 are never updated: give them content, so that a store that strays into them shows
    g["shN"][:, 4:] = np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (N, 20, 3)).astype(np.float32)
    return g


def offset_buffer(a, floats=1):
    """The values of `a` in device memory that starts `floats` floats past a 16-byte boundary."""
    big = torch.zeros(a.size + 4, device="cuda:0")
    out = big[floats:floats + a.size]
    out.copy_(torch.from_numpy(a))
    assert out.data_ptr() % 16 == 4 * floats and out.is_contiguous()
    return out


def run(ctx, N, steps, seed, first_step=1, m0=None, v0=None, zero_block=None, misalign=None):
    """`steps` Adam steps on the GPU and in the oracle from the same gradients.  Returns (params, m, v) of both."""
    from starst3r_amd import ops
    rng = np.random.default_rng(seed)
    g0 = gaussians(N, seed)
    P = {k: dev(v) for k, v in g0.items()}
    ref = {k: v.copy() for k, v in g0.items()}
    m_o = np.zeros(23 * N, np.float32) if m0 is None else m0.copy()
    v_o = np.zeros(23 * N, np.float32) if v0 is None else v0.copy()
    m = offset_buffer(m_o) if misalign == "m" else dev(m_o)
    v = dev(v_o)
    assert all(t.data_ptr() % 16 == 0 for t in P.values()) and v.data_ptr() % 16 == 0
    for step in range(first_step, first_step + steps):
        gr = lac.wide_range_grads(rng, 23 * N)
        if zero_block is not None:
            gr[lac.adam_block_slices(N)[zero_block]] = 0.0
        ops.adam_step(ctx, P, offset_buffer(gr) if misalign == "grads" else dev(gr), m, v, *lac.ADAM_HP, step)
        lac.adam_oracle_step(ref, m_o, v_o, gr, step)
    torch.cuda.synchronize()
    got = ({k: P[k].cpu().numpy() for k in lac.ADAM_NAMES}, m.cpu().numpy(), v.cpu().numpy())
    return got, (ref, m_o, v_o), g0


def check(tag, got, want, g0):
    (P, m, v), (ref, m_o, v_o) = got, want
    worst = max(np.abs(P[k].astype(np.float64) - ref[k]).max() for k in lac.ADAM_NAMES)
    ok = m_o != 0
    rm = (np.abs(m[ok].astype(np.float64) - m_o[ok]) / np.abs(m_o[ok])).max() if ok.any() else 0.0
    ok = v_o != 0
    rv = (np.abs(v[ok].astype(np.float64) - v_o[ok]) / np.abs(v_o[ok])).max() if ok.any() else 0.0
    print(f"ADAM {tag}: parameters {worst:.2e} (3e-7) m {rm:.2e} v {rv:.2e} (relative, 1e-5)")
    for name in lac.ADAM_NAMES:
        np.testing.assert_allclose(P[name], ref[name], rtol=0, atol=3e-7, err_msg=name)
    assert np.array_equal(P["shN"][:, 4:].view(np.int32), g0["shN"][:, 4:].view(np.int32))  # rows 4..23 untouched
    np.testing.assert_allclose(m, m_o, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(v, v_o, rtol=1e-5, atol=1e-20)


# 4096 blocks x 256 threads: k_adam covers 23N scalars, k_adam4 23N / 4 groups; past that the threads loop
@pytest.mark.parametrize("N,steps", [(1, 4), (2, 4), (3, 4), (5, 4),            # k_adam
                                     (4, 4), (8, 4), (332, 4), (336, 4),        # k_adam4
                                     (50_001, 2),                               # k_adam, grid-stride loop
                                     (200_000, 2)])                             # k_adam4, grid-stride loop
def test_adam_vs_oracle(ctx, N, steps):
    if N == 50_001:
        assert N % 4 and 23 * N > 4096 * 256
    if N == 200_000:
        assert N % 4 == 0 and 23 * N // 4 > 4096 * 256
    got, want, g0 = run(ctx, N, steps, seed=N)
    check(f"N={N} {'k_adam4' if N % 4 == 0 else 'k_adam'}", got, want, g0)


@pytest.mark.parametrize("which", ["m", "grads"])
def test_misaligned_buffer_takes_the_scalar_kernel(ctx, which):
    """N % 4 == 0 but one buffer starts 4 bytes past a 16-byte boundary: st3r_adam_impl must fall back to k_adam (k_adam4's
    float4 accesses would be misaligned).  The result meets the oracle like any other.  Whether it is also bit-equal to the
    aligned call's is printed, not asserted: the compiler may contract `v * b2 + (w2 * g) * g` differently in the two
    kernels."""
    N = 336
    got, want, g0 = run(ctx, N, 4, seed=N, misalign=which)
    check(f"N={N} misaligned {which} (k_adam)", got, want, g0)
    aligned, _, _ = run(ctx, N, 4, seed=N)
    eq = {k: np.array_equal(got[0][k].view(np.int32), aligned[0][k].view(np.int32)) for k in lac.ADAM_NAMES}
    eq["m"] = np.array_equal(got[1].view(np.int32), aligned[1].view(np.int32))
    eq["v"] = np.array_equal(got[2].view(np.int32), aligned[2].view(np.int32))
    print(f"ADAM k_adam (misaligned {which}) against k_adam4 (aligned), bit-equal: {eq}")


@pytest.mark.parametrize("N", [333, 336])
def test_zero_gradient_on_zero_state_changes_nothing(ctx, N):
    """One parameter block never receives a gradient and starts with m = v = 0: the update is 0 / (0 + eps) = 0 exactly --
    parameters bit-unchanged, m and v still zero, no NaN -- while the other blocks follow the oracle."""
    got, want, g0 = run(ctx, N, 3, seed=N + 1, zero_block="scales")
    check(f"N={N} zero block", got, want, g0)
    (P, m, v) = got
    sl = lac.adam_block_slices(N)["scales"]
    assert np.array_equal(P["scales"].view(np.int32), g0["scales"].view(np.int32))
    assert np.all(m[sl] == 0) and np.all(v[sl] == 0)
    assert all(np.isfinite(a).all() for a in (*P.values(), m, v))


@pytest.mark.parametrize("N", [333, 336])
def test_late_step_on_warm_state(ctx, N):
    """step = 7000: both bias corrections are within 1e-3 of 1, and m, v carry history.  The drawn state is consistent --
    m = a s, v = (b s)^2 with s the decade of the scalar, |a| ~ 1, b >= 0.5 -- so the update stays of the order of lr, as
    after a real run."""
    rng = np.random.default_rng(70 + N)
    s = 10.0 ** rng.integers(-5, 1, 23 * N)
    m0 = (rng.standard_normal(23 * N) * s).astype(np.float32)
    v0 = (((np.abs(rng.standard_normal(23 * N)) + 0.5) * s) ** 2).astype(np.float32)
    assert (v0 > 0).all() and 1 - 0.999 ** 7000 > 0.999
    got, want, g0 = run(ctx, N, 2, seed=N + 2, first_step=7000, m0=m0, v0=v0)
    check(f"N={N} step 7000 warm", got, want, g0)
