"""Cases, references and predicates shared by test_oracle_exchange_cases.py (CPU pins) and test_gpu_exchange_cases.py: the
gradient exchange of the view-sharded step (csrc/comm.hip) and the range, piece and stage paths of csrc/adam.hip.

One fact carries every check: an exchange form is data movement plus the element-wise Adam that test_gpu_adam.py pins.
Whatever the form, the world and the shape, the result is the float32 sum of the ranks' gradient buffers IN RANK ORDER
(tests/fake_rccl adds in rank order, k_xreduce adds in rank order by construction, two ranks commute), then Adam per element.
From zero moments the first moment decodes that sum exactly: m = fmaf(w1, g - 0, 0) = round32(float32(0.1) g), one exact
product in float64 rounded once.

Host arithmetic restated here, each checked against its source text by the CPU file:
  st3r_adam_impl    k_adam4 exactly if the update is a contiguous range (no Gaussian range, no range-major stage) and
                    N % 4 == 0, i0 % 4 == 0, (i1 - i0) % 4 == 0, sh_stride % 4 == 0 and every buffer 16-byte aligned
  st3r_gs_train_step  rs_ag / direct: q = 23 N / w, tail0 = q w, rank r owns [r q, (r + 1) q), everyone [tail0, 23 N)
                      ranges: K = 4 from N = 4096 on (1 below: the grouped launch), range j = [N j / K, N (j + 1) / K)"""
import functools
import os

import numpy as np

import loss_adam_cases as lac
from st3r_synth import synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "starst3r_amd", "csrc")
BLOCKS = lac.ADAM_BLOCKS + (("shN", 12),)          # the 23N buffer: means 3N, quats 4N, scales 3N, opacities N, SH rows 0..3 12N
FORMS = ("allreduce", "ranges", "rs_ag", "direct")
PIECEWISE = ("rs_ag", "direct")                    # forms under which a rank maintains its piece and the tail only
# test_gpu_adam.check's bounds, the project's own for k_adam / k_adam4 against gso_adam
PARAM_ATOL, M_RTOL, M_ATOL, V_RTOL, V_ATOL = 3e-7, 1e-5, 1e-12, 1e-5, 1e-20
TRAIN_HP = (0.2, 0.01, 0.01)                       # ssim_fac, opac_fac, scale_fac
RANGES_K, RANGES_FROM = 4, 4096                    # EXCH_RANGES_K, the N from which st3r_gs_train_step splits


# ---- the buffer and its pieces ----
def block_starts(N):
    """[0, 3N, 7N, 10N, 11N, 23N]"""
    out = [0]
    for _, w in BLOCKS:
        out.append(out[-1] + w * N)
    return out


def block_of(N, i):
    """(block index, offset inside the block) of buffer index i < 23N"""
    st = block_starts(N)
    assert 0 <= i < st[-1]
    b = max(k for k in range(5) if st[k] <= i)
    return b, i - st[b]


def layout(N, w):
    """(total, q, tail0) of st3r_gs_train_step's rs_ag / direct branches"""
    total = 23 * N
    q = total // w
    return total, q, q * w


def pieces(N, w):
    _, q, _ = layout(N, w)
    return [(r * q, (r + 1) * q) for r in range(w)]


def adam_kernel(N, i0, i1, sh_stride=72, aligned=True, by_gaussian=False):
    """The kernel st3r_adam_impl launches for the range [i0, i1): None (no launch), "k_adam4" or "k_adam"."""
    if i1 - i0 <= 0:
        return None
    contiguous = not by_gaussian
    if contiguous and N % 4 == 0 and i0 % 4 == 0 and (i1 - i0) % 4 == 0 and sh_stride % 4 == 0 and aligned:
        return "k_adam4"
    return "k_adam"


def piece_tags(N, w, sh_stride=72, aligned=True):
    """Per virtual rank: its piece, the kernel the piece must take and the kernel the tail must take."""
    total, _, tail0 = layout(N, w)
    return [dict(rank=r, i0=i0, i1=i1, kernel=adam_kernel(N, i0, i1, sh_stride, aligned),
                 tail_kernel=adam_kernel(N, tail0, total, sh_stride, True))     # (the tail call passes no stage)
            for r, (i0, i1) in enumerate(pieces(N, w))]


def boundaries(N, w):
    """Where the buffer is cut: r q for r = 1 .. w (the last one is tail0), without 0 and 23N.  Each as a dict with the
    block it falls into, whether it lies strictly inside it or exactly on its start, and its position inside a Gaussian's
    twelve SH scalars (0 = between two Gaussians; None outside the SH block)."""
    total, q, _ = layout(N, w)
    out = []
    for b in sorted({r * q for r in range(1, w + 1)} - {0, total}):
        k, off = block_of(N, b)
        out.append(dict(at=b, block=BLOCKS[k][0], inside=off > 0, on_block_start=off == 0,
                        sh_pos=(off % 12 if k == 4 else None)))
    return out


def ranges(N):
    """(K, [(g0, g1)]) of the range-wise form"""
    K = RANGES_K if N >= RANGES_FROM else 1
    return K, [(N * j // K, N * (j + 1) // K) for j in range(K)]


# ---- part 1: pieces and stages in one process ----
PIECE_CASES = [(1, 2), (1, 4), (1, 8), (3, 64), (2, 64), (5, 3), (333, 7), (336, 3), (336, 4), (336, 8), (1003, 4),
               # added for the tail lengths of w = 8 (23 N mod 8 = 8 - N mod 8): 6, 5, 4, 3, 2, 1
               (2, 8), (3, 8), (4, 8), (5, 8), (6, 8), (7, 8)]


def piece_gaussians(N, seed, compact_sh=False):
    """Parameters with content in SH rows 4..23 (a store that strays into them shows); compact_sh: the four used rows
    alone, [N, 4, 3] (sh_stride 12)"""
    g = synth.make_gaussians(N, seed=seed)
    g = {k: g[k] for k in lac.ADAM_NAMES}
    g["shN"][:, 4:] = np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (N, 20, 3)).astype(np.float32)
    if compact_sh:
        g["shN"] = np.ascontiguousarray(g["shN"][:, :4])
    return g


def foreign_moments(N, w, rank, seed):
    """(m, v, keep) a virtual rank starts from: zero on its piece and on the tail (as after the form's first attach),
    drawn and non-zero everywhere else -- `keep` is that mask: these must keep their bits, the rank does not own them."""
    total, q, tail0 = layout(N, w)
    rng = np.random.default_rng(seed * 1000 + rank)
    m = (rng.standard_normal(total) + 3.0).astype(np.float32)
    v = (rng.uniform(0.5, 2.0, total)).astype(np.float32)
    keep = np.ones(total, bool)
    keep[rank * q:(rank + 1) * q] = False
    keep[tail0:] = False
    m[~keep] = 0.0
    v[~keep] = 0.0
    assert (m[keep] != 0).all() and (v[keep] != 0).all()
    return m, v, keep


@functools.lru_cache(maxsize=None)
def piece_reference(N, w, steps=2, compact_sh=False):
    """The oracle's Adam (gso_adam through loss_adam_cases.adam_oracle_step) on the WHOLE buffer from zero moments, `steps`
    steps of wide_range_grads: a list per step of (gradient, parameters, m, v) and the start.  Computed once per shape."""
    seed = 100 * N + w
    rng = np.random.default_rng(seed)
    g0 = piece_gaussians(N, seed, compact_sh)
    ref = {k: a.copy() for k, a in g0.items()}
    m_o = np.zeros(23 * N, np.float32); v_o = np.zeros(23 * N, np.float32)
    out = []
    for step in range(1, steps + 1):
        gr = lac.wide_range_grads(rng, 23 * N)
        lac.adam_oracle_step(ref, m_o, v_o, gr, step)
        out.append((gr, {k: a.copy() for k, a in ref.items()}, m_o.copy(), v_o.copy()))
    return dict(g0=g0, steps=out, seed=seed)


def over_bounds(p, m, v, p_o, m_o, v_o):
    """(parameters, m, v): the largest error in units of its bound (<= 1 passes test_gpu_adam.check)"""
    def rel(a, b, rtol, atol):
        a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
        return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max()) if a.size else 0.0
    return (rel(p, p_o, 0.0, PARAM_ATOL), rel(m, m_o, M_RTOL, M_ATOL), rel(v, v_o, V_RTOL, V_ATOL))


def assert_check_bounds(tag, p, m, v, p_o, m_o, v_o):
    """test_gpu_adam.check on flat arrays (numpy's own closeness test, the same tolerances)"""
    np.testing.assert_allclose(p, p_o, rtol=0, atol=PARAM_ATOL, err_msg=f"{tag}: parameters")
    np.testing.assert_allclose(m, m_o, rtol=M_RTOL, atol=M_ATOL, err_msg=f"{tag}: m")
    np.testing.assert_allclose(v, v_o, rtol=V_RTOL, atol=V_ATOL, err_msg=f"{tag}: v")


# ---- parts 2 and 3: whole steps on small scenes ----
VIEW_W, VIEW_H = 48, 32
RANGE_NS = (4095, 4096, 4097, 4098, 4099)
WORLDS = (2, 3, 4)
WORLD_CASES = tuple((str(n), n, False) for n in (1, 2, 3, 5) + RANGE_NS) + (("5_away", 5, True),)   # (name, N, last rank sees nothing)


def scene(N, world, away=False):
    """(gaussians, w2c [world,4,4], Ks, gt [world,H,W,3]): one 48 x 32 view per rank of a synthetic scene; the ground
    truth is noise (the checks are about where sums go, not about what is learnt).  away: the last camera keeps its place
    and looks away from the scene: no Gaussian in front of it, its gradient is the two regularisers'."""
    few = N < 100
    g = synth.make_gaussians(N, seed=4000 + N, scale_lo=0.05 if few else 0.01, scale_hi=0.3 if few else 0.05,
                             extent=0.5 if few else 1.0)
    g = {k: g[k] for k in lac.ADAM_NAMES}
    g["shN"][:, 4:] = np.random.default_rng(N + 1).uniform(-0.5, 0.5, (N, 20, 3)).astype(np.float32)
    w2c, Ks = synth.make_cameras(world, VIEW_W, VIEW_H)
    if away:
        eye = np.linalg.inv(w2c[-1].astype(np.float64))[:3, 3]
        w2c[-1] = synth.look_at_w2c(eye, target=2 * eye).astype(np.float32)
    gt = np.random.default_rng(7 * N + world).uniform(0, 1, (world, VIEW_H, VIEW_W, 3)).astype(np.float32)
    return g, w2c, Ks, gt


def pack(P):
    """parameter dict (numpy) -> the 23N floats in buffer order"""
    N = P["means"].shape[0]
    return np.concatenate([np.asarray(P[k]).reshape(-1) for k, _ in lac.ADAM_BLOCKS] +
                          [np.ascontiguousarray(np.asarray(P["shN"])[:, :4]).reshape(-1)]).astype(np.float32, copy=False) \
        if N else np.zeros(0, np.float32)


def unpack(buf):
    """23N floats -> parameter dict with the four used SH rows, [N, 4, 3] (copies)"""
    N = buf.size // 23
    sl = lac.adam_block_slices(N)
    out = {k: buf[sl[k]].copy().reshape((N, w) if w > 1 else (N,)) for k, w in lac.ADAM_BLOCKS}
    out["shN"] = buf[sl["shN"]].copy().reshape(N, 4, 3)
    return out


def rank_ordered_sum(gs):
    """((g_0 + g_1) + g_2) + ... in float32"""
    S = np.asarray(gs[0], np.float32).copy()
    for g in gs[1:]:
        S = (S + np.asarray(g, np.float32)).astype(np.float32)
    return S


def first_moment_bits(S):
    """Bits of the first moment after one step from zero moments: fmaf(w1, S - 0, 0) with w1 = float32(1 - 0.9): one exact
    float64 product (24 x 24 bits) rounded once; -0 + 0 = +0 like the fma's addend"""
    w1 = np.float64(np.float32(1.0 - lac.ADAM_HP[1]))
    return (w1 * S.astype(np.float64) + 0.0).astype(np.float32).view(np.int32)


def oracle_step(p, m, v, g, step):
    """adam_oracle_step on packed buffers (copies): -> (parameters, m, v)"""
    ref = unpack(np.asarray(p, np.float32)); m_o = np.array(m, np.float32); v_o = np.array(v, np.float32)
    lac.adam_oracle_step(ref, m_o, v_o, np.asarray(g, np.float32), step)
    return pack(ref), m_o, v_o


def owned(N, w, rank):
    """mask of the scalars rank `rank` maintains under rs_ag / direct: its piece and the tail"""
    total, q, tail0 = layout(N, w)
    own = np.zeros(total, bool)
    own[rank * q:(rank + 1) * q] = True
    own[tail0:] = True
    return own
