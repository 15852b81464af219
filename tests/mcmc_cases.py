"""Hand-built inputs for the MCMC refinement kernels (csrc/mcmc.hip + csrc/scan.h), their float64 references and their
bounds.  test_oracle_mcmc_cases.py pins every case on oracle/mcmc_oracle.py alone (no GPU); test_gpu_mcmc_cases.py
runs them through `ops`.

Where the numbers come from
  * integer state (weights, prefix sums, ranks, draws, counts): equality.  Opacity logits 20 / 0 / -200 have float32
    sigmoids of exactly 1 / 0.5 / 0 in any conforming evaluation of 1 / (1 + expf(-x)) (expf(-20) < 2^-24 is absorbed
    by the addition, expf(0) == 1, expf(200) == inf), so the fixed-point weights are exactly 2^24 / 2^23 / 0 and the
    prefix sums have a closed form that never touches the device.
  * relocated opacity and scale: `reloc_bound` = max(4 x |float32 oracle - float64 closed form|, floor) per source,
    on the stored values (a logit and a LOG scale: a relative error of the scale factor is an absolute error there).
    The floor is a first-order forward error bound of the kernel's formula with the documented accuracy of the device
    library (HIP math API: expf, logf, powf 1 ulp; +, *, /, sqrtf correctly rounded), see `reloc_reference`.  A source
    whose floor exceeds 1 (the sign of the scale factor is not determined by float32 arithmetic) is OUTSIDE the domain of
    the float32 formula: there the kernel and the oracle are only asked to agree in sign and finiteness.
  * noise: `noise_bound` = max(4 x |float32 numpy restatement - float64 oracle|, floor) per element, the floor relative
    to the row's largest component: 1e-6 plus the derived error of the gate, which multiplies the rounding of
    1 - sigmoid(o) by 100 (see `noise_bound`).
"""
import math

import numpy as np

from oracle import mcmc_oracle as mo

F = np.float32
U = 2.0 ** -24           # unit round-off of binary32 (correctly rounded operation)
ULP = 2.0 ** -23         # documented 1-ulp bound of expf / logf / powf, relative
TILE = 2048              # st3r_scan::TILE
L_ONE, L_HALF, L_ZERO = F(20.0), F(0.0), F(-200.0)
_BINOMS = mo.binom_table()
EXACT_N = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 524288, 524289)


# ------------------------------------------------------------------------------------------------- parameters
def params(N, logits, shN_rows=4, sh0=True, seed=0, scales=None, quats=None):
    """Distinct, reproducible rows: every float identifies its (row, column), so a copy from the wrong row shows."""
    rng = np.random.default_rng(seed + 1000)
    P = {"means": rng.normal(size=(N, 3)), "quats": rng.normal(size=(N, 4)) if quats is None else quats,
         "scales": rng.normal(-4, 0.3, (N, 3)) if scales is None else scales, "opacities": np.asarray(logits),
         "shN": rng.normal(size=(N, shN_rows, 3))}
    if sh0:
        P["sh0"] = rng.normal(size=(N, 1, 3))
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in P.items()}


# ------------------------------------------------------------------------------------------------- 1. exact weights
def exact_logits(N):
    """Pattern of the three exact values.  Zeros at 0, N - 1, on both sides of every tile edge, in a run of 300 and
    (N <= 4097) at every 13th index; the rest alternates 1 and 0.5 irregularly."""
    i = np.arange(N)
    cls = ((i * 7 + i // 5 + i // 2048) % 3 == 0).astype(np.int64)      # 1: half, 0: one
    zero = np.zeros(N, bool)
    if N > 1:
        zero[0] = True; zero[N - 1] = True
    for e in range(TILE, N + 1, TILE):
        zero[e - 1] = True
        if e < N:
            zero[e] = True
    if N >= 2047:
        zero[900:1200] = True
    if 2 < N <= 4097:
        zero[::13] = True
    if N == 2:
        zero[:] = [True, False]
    lg = np.where(cls == 1, L_HALF, L_ONE).astype(F)
    lg[zero] = L_ZERO
    return lg


def exact_weights(logits):
    """Closed form, no sigmoid evaluated."""
    w = np.zeros(len(logits), np.uint64)
    w[logits == L_ONE] = 1 << 24; w[logits == L_HALF] = 1 << 23
    assert ((logits == L_ONE) | (logits == L_HALF) | (logits == L_ZERO)).all()
    return w


def exact_case(N):
    lg = exact_logits(N)
    return dict(N=N, P=params(N, lg, shN_rows=4, seed=N), w=exact_weights(lg), min_opacity=0.25,
                n_new=3 if N < 255 else 200, seed=0x1234567ABCDEF, step=N % 97)


# ------------------------------------------------------------------------------------------------- 2. plateaus
def plateau_logits():
    """N = 64: a leading zero weight, interior runs of zeros, trailing zeros (the add path: nobody is dead, a zero
    weight is a sigmoid of exactly 0)."""
    lg = np.where(np.arange(64) % 2 == 0, L_ONE, L_HALF).astype(F)
    for a, b in ((0, 1), (5, 6), (9, 13), (31, 33), (40, 52), (60, 64)):
        lg[a:b] = L_ZERO
    return lg


def tiny_logits():
    """N = 64 with weights of 1 (logit -16: sigmoid 2^24 = 1.89), 5 (logit -15: 5.13) and 0: the total is about 100, so
    nearly every draw t EQUALS a prefix sum -- the one input on which `cum[mid] > t` and `>=` pick different sources
    (with 24-bit weights of ordinary opacities a draw hits a prefix sum with probability 2^-24)."""
    lg = np.where(np.arange(64) % 3 == 0, F(-15.0), F(-16.0)).astype(F)
    for a, b in ((0, 2), (10, 11), (20, 25), (62, 64)):
        lg[a:b] = L_ZERO
    return lg


# ------------------------------------------------------------------------------------------------- 3./4. forced ratios
def single_source(logit, n_dead, log_scales=(-4.0, -3.5, -5.0), dead_logit=-200.0, seed=1):
    """Row 0 alive with `logit`, rows 1..n_dead dead: every draw picks row 0, count = n_dead, ratio n_dead + 1."""
    N = 1 + n_dead
    lg = np.full(N, dead_logit, F); lg[0] = logit
    sc = np.tile(np.asarray(log_scales, F), (N, 1))
    return params(N, lg, shN_rows=4, seed=seed, scales=sc)


def two_sources():
    """Two alive sources of different weight in one call (logits 20 and -3: sigmoids 1 and 0.047) and 60 dead rows: the
    draws split unevenly, two different ratios are applied in one launch."""
    N = 62
    lg = np.full(N, -200.0, F); lg[7] = 20.0; lg[40] = -3.0
    return params(N, lg, shN_rows=4, seed=5)


GRID_O = (0.006, 0.1, 0.5, 0.9, 0.99, 1 - 2.0 ** -13, 1 - 2.0 ** -23)
GRID_RATIO = (2, 5, 20, 51)


def logit_of(o):
    return F(math.log(o / (1.0 - o)))


def sigmoid_is_robust(logit):
    """float32 sigmoid of `logit` with expf off by up to 2 ulp either way: the same float for all of them?"""
    with np.errstate(over="ignore"):
        e = np.exp(-F(logit), dtype=F)
    outs = {float(F(1) / (F(1) + F(float(e) * (1 + k * ULP)))) for k in (-2, -1, 0, 1, 2)}
    return len(outs) == 1


# float64 evaluation of the closed form, written independently of oracle.compute_relocation ---------------------------
def _denominator64(no, n):
    """sum_{i=1..n} sum_{k<i} C(i-1,k) (-1)^k no^(k+1) / sqrt(k+1) with exact binomials; also sum |terms|, the
    derivative with respect to `no` and the sum of the running partial sums' magnitudes in the kernel's order."""
    terms = []
    for i in range(1, n + 1):
        for k in range(i):
            terms.append((math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1), k + 1))
    vals = [c * no ** p for c, p in terms]
    D = math.fsum(vals)
    dD = math.fsum(c * p * no ** (p - 1) for c, p in terms)
    run, acc = 0.0, 0.0
    for v in vals:
        acc += v; run += abs(acc)
    return D, math.fsum(abs(v) for v in vals), dD, run


def reloc_reference(logit, log_scale, ratio, min_opacity):
    """float64 (new logit, new log scale [3], floor_logit, floor_logscale) of one source.  The floors are first-order
    forward error bounds of k_mcmc_update_sources' float32 evaluation: every +, *, / contributes U = 2^-24 relative,
    every expf / powf / logf ULP = 2^-23 relative (documented 1 ulp), propagated through the float64 derivatives."""
    n = int(min(max(int(ratio), 1), mo.NMAX))
    x = float(F(logit))
    e = math.exp(-x)
    o = 1.0 / (1.0 + e)
    # sigmoid: expf 1 ulp, the addition and the division half an ulp each
    d_o = o * ((e * ULP + U * (1.0 + e)) / (1.0 + e) + U)
    o32 = float(mo.sigmoid32(F(logit)))
    if sigmoid_is_robust(logit):
        o, d_o = o32, 0.0          # every conforming float32 sigmoid returns this very float
    a = 1.0 - o
    d_a = d_o + (U * a if o < 0.5 else 0.0)           # Sterbenz: exact for o >= 0.5
    inv_n = float(F(1.0) / F(n))
    if a == 0.0:
        p, d_p = 0.0, 0.0                             # powf(0, y > 0) == 0 exactly
    else:
        p = a ** inv_n
        d_p = p * ULP + p * inv_n * d_a / a
    no = 1.0 - p
    d_no = d_p + U * no
    D, sum_abs, dD, run = _denominator64(no, n)
    # per term: powf 1 ulp, sqrtf / division / two products half an ulp each; per partial sum half an ulp
    d_D = sum_abs * (ULP + 4 * U) + abs(dD) * d_no + U * run
    coeff = o / D
    rel_coeff = (d_o / o if o else 0.0) + d_D / abs(D) + U
    new_ls = np.log(abs(coeff)) + np.asarray(log_scale, np.float64)
    # logf(coeff * expf(ls)): expf 1 ulp, product half, logf 1 ulp of the result
    floor_ls = rel_coeff + ULP + U + ULP * np.abs(new_ls).max()
    lo, hi = float(F(min_opacity)), float(F(1) - mo.F32_EPS)
    c = min(max(no, lo), hi)
    d_c = d_no if (lo + d_no < no < hi - d_no) else (0.0 if (no < lo - d_no or no > hi + d_no) else d_no)
    new_logit = math.log(c / (1.0 - c))
    floor_logit = d_c / c + (d_c + U * (1 - c)) / (1.0 - c) + U + ULP * abs(new_logit)
    return new_logit, new_ls, floor_logit, float(floor_ls), coeff


def reloc_bound(logit, log_scale, ratio, min_opacity):
    """(ref_logit, ref_logscale[3], bound_logit, bound_logscale, yard_logit, yard_logscale, in_domain) of one source:
    yard = the float32 oracle's own error, bound = max(4 yard, floor)."""
    ref_lg, ref_ls, fl_lg, fl_ls, coeff = reloc_reference(logit, log_scale, ratio, min_opacity)
    with np.errstate(all="ignore"):      # the float32 oracle on this one source (mo._apply_sources with a cached table)
        no32, ns32 = mo.compute_relocation(mo.sigmoid32(np.array([logit], F)),
                                           np.exp(np.asarray(log_scale, F).reshape(1, 3), dtype=F),
                                           np.array([int(ratio)]), _BINOMS)
        no32 = np.clip(no32, F(min_opacity), F(1) - mo.F32_EPS)
        P = {"opacities": np.log(no32 / (F(1) - no32), dtype=F), "scales": np.log(ns32, dtype=F)}
    in_domain = fl_ls < 1.0
    y_lg = abs(float(P["opacities"][0]) - ref_lg)
    y_ls = float(np.abs(P["scales"][0].astype(np.float64) - ref_ls).max()) if in_domain else float("inf")
    return dict(ref_logit=ref_lg, ref_logscale=ref_ls, bound_logit=max(4 * y_lg, fl_lg),
                bound_logscale=max(4 * y_ls, fl_ls), yard_logit=y_lg, yard_logscale=y_ls, floor_logit=fl_lg,
                floor_logscale=fl_ls, in_domain=in_domain, oracle_logit=float(P["opacities"][0]),
                oracle_logscale=P["scales"][0].copy(), coeff=coeff)


def denominator32_at_one(n, fused):
    """The float32 denominator at new opacity == 1 (sigmoid == 1.0f) in the kernel's order: product and sum rounded
    separately (`fused=False`: the oracle, and the kernel with contraction off) or as one fused multiply-add, rounded
    exactly (what the compiler makes of `denom += b * t` when it may contract)."""
    from fractions import Fraction

    def round32(fr):
        f = F(float(fr))
        return min((f, np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))), key=lambda c: abs(Fraction(float(c)) - fr))
    d = F(0)
    for i in range(1, n + 1):
        for k in range(i):
            coef = F((-1.0) ** k) / np.sqrt(F(k + 1))
            if fused:
                d = round32(Fraction(float(_BINOMS[i - 1, k])) * Fraction(float(coef)) + Fraction(float(d)))
            else:
                d = F(d + _BINOMS[i - 1, k] * coef)
    return float(d)


def check_sources(P_in, got, uniq, counts, min_opacity):
    """Per-source comparison of the stored logit and log scales with the float64 reference within `reloc_bound`;
    outside the domain: same sign and finiteness as the float32 oracle.  Returns the worst error / bound."""
    worst = 0.0
    for g, c in zip(uniq, counts):
        b = reloc_bound(P_in["opacities"][g], P_in["scales"][g], int(c) + 1, min_opacity)
        e_lg = abs(float(got["opacities"][g]) - b["ref_logit"])
        assert e_lg <= b["bound_logit"], ("logit", int(g), int(c), e_lg, b["bound_logit"])
        worst = max(worst, e_lg / b["bound_logit"])
        gs = got["scales"][g].astype(np.float64)
        if b["in_domain"]:
            e_ls = float(np.abs(gs - b["ref_logscale"]).max())
            assert e_ls <= b["bound_logscale"], ("log scale", int(g), int(c), e_ls, b["bound_logscale"])
            worst = max(worst, e_ls / b["bound_logscale"])
        else:
            assert (np.isfinite(gs) == np.isfinite(b["oracle_logscale"])).all(), (int(g), gs, b["oracle_logscale"])
            assert (np.isnan(gs) == np.isnan(b["oracle_logscale"])).all(), (int(g), gs, b["oracle_logscale"])
    return worst


def check_relocated(P_in, got, sampled, dst_ids, min_opacity):
    """Everything a relocation / growth may change, nothing masked: sources within their bound (opacity, scales) and
    bit-equal elsewhere; destination rows bit-equal to their source's rows of `got`; every other row bit-equal to the
    input.  `got` holds at least the rows of P_in (growth: more).  Returns worst error / bound over the sources."""
    N = P_in["means"].shape[0]
    sampled = np.asarray(sampled, np.int64); dst_ids = np.asarray(dst_ids, np.int64)
    uniq, counts = np.unique(sampled, return_counts=True)
    worst = check_sources(P_in, got, uniq, counts, min_opacity)
    touched = np.zeros(N, bool); touched[uniq] = True; touched[dst_ids[dst_ids < N]] = True
    for k in P_in:
        g = got[k]
        np.testing.assert_array_equal(g[:N][~touched].view(np.uint32), P_in[k][~touched].view(np.uint32), err_msg=k)
        np.testing.assert_array_equal(g[dst_ids].view(np.uint32), g[sampled].view(np.uint32), err_msg=k)
        if k not in ("opacities", "scales"):
            np.testing.assert_array_equal(g[uniq].view(np.uint32), P_in[k][uniq].view(np.uint32), err_msg=k)
    return worst


# ------------------------------------------------------------------------------------------------- 6. noise
def noise_case(N, seed=0):
    """means = 0 (the output IS the increment); quaternion norms 1e-3 .. 1e3, log scales -8 .. 1, logits -9 .. 9 (the
    gate sweeps from ~1 to exactly 0).  Logits whose float32 gate would be subnormal (expf argument within 87 .. 89.5,
    just below the overflow to inf) are moved up by 0.3: whether a subnormal quotient is kept is not part of the
    contract being checked."""
    rng = np.random.default_rng(77 + N + seed)
    q = rng.normal(size=(N, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= 10.0 ** np.linspace(-3, 3, N)[rng.permutation(N)][:, None]
    sc = np.stack([np.linspace(-8, 1, N)[rng.permutation(N)] for _ in range(3)], -1)
    lg = np.linspace(-9, 9, N) if N > 1 else np.array([-3.0])
    lg = lg.astype(F)
    arg = gate_arg32(lg)
    lg = np.where((arg > 87.0) & (arg < 89.5), lg + F(0.3), lg).astype(F)
    P = params(N, lg, shN_rows=4, seed=N, scales=sc, quats=q)
    P["means"][:] = 0
    return P


def gate_arg32(logits):
    """The float32 argument of the gate's expf: -100 ((1 - op) - 0.995)."""
    op = mo.sigmoid32(logits)
    return (F(-100.0) * ((F(1) - op) - F(0.995))).astype(F)


def noise_f32(quats, scales, opacities, scaler, step, seed, row_offset=0):
    """float32 numpy restatement of k_mcmc_noise's formula, operation by operation (no contraction)."""
    n = len(opacities)
    r = mo.philox4x32_10(np.arange(n, dtype=np.uint64) + np.uint64(row_offset), 0, mo.STREAM_NOISE, step,
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = [((x >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0) for x in r]
    two_pi = F(6.283185307179586)
    ra = np.sqrt(F(-2) * np.log(u[0])); rb = np.sqrt(F(-2) * np.log(u[2]))
    nz = [ra * np.cos(two_pi * u[1]), ra * np.sin(two_pi * u[1]), rb * np.cos(two_pi * u[3])]
    op = mo.sigmoid32(opacities)
    with np.errstate(over="ignore"):
        gate = F(1) / (F(1) + np.exp(F(-100) * ((F(1) - op) - F(0.995)), dtype=F))
    k = gate * F(scaler)
    q = np.asarray(quats, F)
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    inv = F(1) / np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    qw, qx, qy, qz = qw * inv, qx * inv, qy * inv, qz * inv
    two, one = F(2), F(1)
    R = [one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy),
         two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx),
         two * (qx * qz - qw * qy), two * (qy * qz + qw * qx), one - two * (qx * qx + qy * qy)]
    s = np.exp(np.asarray(scales, F))
    t = [(R[j] * nz[0] + R[3 + j] * nz[1] + R[6 + j] * nz[2]) * k * s[:, j] * s[:, j] for j in range(3)]
    out = np.stack([R[3 * i] * t[0] + R[3 * i + 1] * t[1] + R[3 * i + 2] * t[2] for i in range(3)], -1)
    assert out.dtype == F
    return out


def normals_at(rows, step, seed):
    """oracle.normals for arbitrary global rows (float64)."""
    r = mo.philox4x32_10(np.asarray(rows, np.uint64), 0, mo.STREAM_NOISE, step, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = [(((x >> np.uint32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)).astype(np.float64) for x in r]
    ra = np.sqrt(-2.0 * np.log(u[0])); rb = np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]), rb * np.cos(2 * np.pi * u[3])], -1)


def noise_bound(P, scaler, step, seed):
    """(want float64 [N,3], bound [N,3], yard [N,3], exact_zero [N]).

    bound = max(4 |float32 restatement - float64|, floor, 2^-126), floor = M (1e-6 + rel_gate), M = the row's largest
    |want|.
    rel_gate, derived: gate = 1 / (1 + expf(a)), a = -100 ((1 - op) - 0.995).  op carries at most 3 U absolute (expf
    1 ulp, +, / half each, op <= 1); 1 - op and the subtraction of 0.995 add U each, the product U |a|:
        |da| <= 100 (3 U + 2 U) + U |a|
    and d gate / gate = (1 - gate) (da + ULP) + 2 U (expf's own ulp, the addition, the division).  At op -> 1 this is
    about 600 U = 3.6e-5; at op -> 0 the factor (1 - gate) removes it: the bound grows with the opacity.
    exact_zero: rows whose expf argument exceeds ln(FLT_MAX) = 88.7228 by a margin: expf == inf, gate == 0 and the
    increment is exactly 0 in float32 whatever the other factors are."""
    want = mo.noise_delta(P["quats"], P["scales"], P["opacities"], scaler, step, seed)
    f32 = noise_f32(P["quats"], P["scales"], P["opacities"], scaler, step, seed).astype(np.float64)
    yard = np.abs(f32 - want)
    op = 1.0 / (1.0 + np.exp(-P["opacities"].astype(np.float64)))
    a = -100.0 * ((1.0 - op) - 0.995)
    gate = 1.0 / (1.0 + np.exp(a))
    rel_gate = (1.0 - gate) * (100 * 5 * U + U * np.abs(a) + ULP) + 2 * U
    M = np.abs(want).max(1)
    floor = (M * (1e-6 + rel_gate))[:, None]
    exact_zero = gate_arg32(P["opacities"]) > 89.5
    # a result below the normal range is quantised absolutely (2^-149 with subnormals kept, flushed to 0 at worst):
    # the relative floor means nothing there, the smallest normal number 2^-126 bounds either behaviour
    return want, np.maximum(np.maximum(4 * yard, floor), 2.0 ** -126), yard, exact_zero
