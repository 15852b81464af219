"""Inputs and float64 references shared by the CPU pins (tests/test_oracle_nn.py) and the GPU parity tests
(tests/test_gpu_nn.py) of path A, csrc/recip_nn.hip: the (n, m) shapes with the kernel paths they are there for, the
descriptor builders (self match, all-negative scores, unnormalised, duplicated rows, planted single answers) and the
reciprocal-loop scenes.  Every (builder, shape) pair listed here is all-clear on the CPU (nn_oracle.clear_queries), so
the GPU tests compare every query; test_oracle_nn.py asserts that, and asserts through st3r_nn_plan that the shapes
still reach the paths named below when the segment heuristic is retuned."""
import functools

import numpy as np

from oracle import nn_oracle as no

D = 24

# (n queries, m rows).  Plans under the present heuristic (S segments of tps tiles):
CASES = [
    (1, 1), (1, 3), (5, 4), (33, 5), (64, 31), (65, 32), (31, 33),      # no full tile / exactly one / one + 1 row
    (63, 64), (129, 65), (70, 96), (32, 97), (70, 127), (70, 128),      # S = 1, tps 2 .. 4
    (70, 129), (70, 160), (70, 161),                                    # S = 2, tps = 3
    (70, 385), (70, 415),                                               # S = 4, the last segment is the ragged tile alone
    (70, 416),
    (200, 2049),                                                        # S = 17
    (64, 4231), (1, 4231),                                              # S = 34: 68 partials, two ballot chunks
    (4231, 4231),                                                       # 67 query groups
    (4231, 9760),                                                       # tps = 5
    (8192, 7168),                                                       # tps = 7, S = 32
]
LARGE = [(4231, 9760), (8192, 7168)]


def plan(n, m):
    """(S, tiles_per_seg) of st3r_nn_plan -- host arithmetic, no GPU."""
    import ctypes as C
    from starst3r_amd import _lib
    S, tps = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().st3r_nn_plan(n, m, C.byref(S), C.byref(tps)))
    return S.value, tps.value


def segments(m, S, tps):
    """[(full tiles, has the ragged tile)] per segment, as k_nn_argmax cuts them (tile0, full1, tile1)."""
    tiles = (m + 31) // 32
    out = []
    for seg in range(S):
        tile0 = seg * tps
        tile1 = min(tile0 + tps, tiles)
        full1 = min(tile1, m // 32)
        out.append((max(full1 - tile0, 0), tile1 > max(full1, tile0)))
    return out


def unit(rng, k):
    x = rng.standard_normal((k, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- builders: (queries [n,24], db [m,24]) float32, deterministic in their arguments ----

def self_match(n, m):
    """Random unit rows, query i IS row i % m: every row of every tile, half-wave, segment and ragged position wins."""
    d = unit(np.random.default_rng(1000 + m), m)
    return d[np.arange(n) % m].copy(), d


def all_negative(n, m):
    """Every score is negative, so a zero-padded row of the ragged tile (score exactly 0) would win if it were let in."""
    rng = np.random.default_rng(2000 + n + m)
    d = (np.abs(rng.standard_normal((m, D))) + 0.1).astype(np.float32)
    q = (-37.0 * (np.abs(rng.standard_normal((n, D))) + 0.1)).astype(np.float32)
    return q, d


def unnormalised(n, m):
    """Mixed sign, every row and every query scaled by its own uniform(0.01, 100) factor."""
    rng = np.random.default_rng(3000 + n + m)
    d = (rng.standard_normal((m, D)) * rng.uniform(0.01, 100, (m, 1))).astype(np.float32)
    q = (rng.standard_normal((n, D)) * rng.uniform(0.01, 100, (n, 1))).astype(np.float32)
    return q, d


def duplicated(n, m0, r):
    """m0 distinct unit rows repeated r times (row j again at j + m0, j + 2 m0, ...): exact ties, the first must win."""
    rng = np.random.default_rng(4000 + n + m0 + r)
    base = unit(rng, m0)
    return unit(rng, n), np.tile(base, (r, 1))


def planted(n, m, row):
    """n distinct queries near one direction u, db[row] = 3 u among random unit rows: every answer is `row`."""
    rng = np.random.default_rng(5000 + n + m + row)
    d = unit(rng, m)
    u = unit(rng, 1)[0]
    q = (u[None, :] + 0.05 * rng.standard_normal((n, D))).astype(np.float32)
    d[row] = 3.0 * u
    return q, d


SELF_MATCH = [(m, m) for m in (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 129, 4231)] + LARGE
RAGGED_M = sorted({m for _, m in CASES if m % 32})
ALL_NEGATIVE = [(70, m) for m in RAGGED_M]
# random scores: the smallest best-to-runner-up gap of n queries over m rows shrinks like 1 / (n m), and from ~1e7
# pairs on some query falls inside the float32 margin (one of 4231 at 4231 x 4231); the shapes above 200 x 2049 are
# reached by the self-match and duplicated-row inputs instead
UNNORMALISED = [c for c in CASES if c[0] * c[1] <= 200 * 2049]
# (n, m0, r) -> what the repeats reach
DUPLICATED = [
    (130, 8, 2),      # rows j, j + 8: the same lane's partial, ragged walk
    (130, 8, 4),      # the same, through the full-tile walk (m = 32)
    (130, 4, 2),      # rows j, j + 4: the two half-waves of a tile
    (130, 32, 3),     # across the tiles of one segment (strict > in the walk)
    (130, 37, 3),     # repeats in the ragged tile
    (130, 1000, 5),   # across segments
    (64, 4231, 2),    # across the ballot chunks of wave_resolve (2 S > 64)
]
PLANTED = [(n, m, row) for n in (1, 65) for m in (33, 416, 4231) for row in (0, m - 1)]

BUILDERS = {"self": self_match, "neg": all_negative, "unnorm": unnormalised, "dup": duplicated, "planted": planted}
FAMILIES = {"self": SELF_MATCH, "neg": ALL_NEGATIVE, "unnorm": UNNORMALISED, "dup": DUPLICATED, "planted": PLANTED}


@functools.lru_cache(maxsize=None)
def reference(family, args):
    """(q, d, idx, best, clear) for BUILDERS[family](*args): float64 arg-max, its score and nn_oracle.clear_queries.
    For the duplicated rows the arg-max and the runner-up are taken over the distinct base rows: inside the full db the
    runner-up of every query is the winner's own copy, and the answer has to be the first copy."""
    q, d = BUILDERS[family](*args)
    db = d[:args[1]] if family == "dup" else d
    idx, best, second = no.nn_dot(q, db, block=1024, dtype=np.float64)
    clear = no.clear_queries(q, db, best, second)
    for a in (q, d, idx, best, clear):
        a.setflags(write=False)
    return q, d, idx, best, clear


def score_bound(q, d, idx):
    """24 * 2^-24 * sum_k |q_k d_k| of the chosen row: the worst-case error of a 24-term float32 dot product, every
    product and every partial sum rounded once (fused multiply-adds and other sum orders only do better)."""
    return 24 * 2.0 ** -24 * np.abs(q.astype(np.float64) * d[idx].astype(np.float64)).sum(1)


# ---- reciprocal loop ----
# name -> (A (H, W, seed), B (H, W, seed) or a crop (h, w) of A's own partner map, subsample)
LOOP_CASES = {
    "1536_seeds": ((64, 96, 3), None, 2),            # two chunks of k_nn_compact
    "1024_seeds": ((32, 32, 5), None, 1),            # exactly one chunk
    "1025_seeds": ((25, 41, 5), None, 1),            # one chunk and one seed
    "cropped_B": ((48, 64, 3), (40, 56), 4),         # SA = 24, SB = 18
    "two_scenes": ((33, 47, 7), (29, 61, 8), 3),     # unrelated sizes, both with a ragged tile
}
LOOP_ITERS = (1, 2, 10)
# converged seeds after 1 / 2 / 10 iterations in the float64 oracle, of the seed count in the last column
LOOP_CONVERGED = {
    "1536_seeds": (838, 1491, 1536, 1536),
    "1024_seeds": (566, 992, 1024, 1024),
    "1025_seeds": (566, 1000, 1025, 1025),
    "cropped_B": (100, 187, 192, 192),
    "two_scenes": (80, 163, 176, 176),
}
# the older loop tests' scenes: synth_descriptors(H, W, planted, seed) with subsample S
VS_ORACLE = [((48, 64), 4), ((96, 128), 8)]


@functools.lru_cache(maxsize=None)
def loop_scene(name):
    (H, W, seed), b, S = LOOP_CASES[name]
    A, B, _, _ = no.synth_descriptors(H, W, planted=0.3, seed=seed)
    if b is not None and len(b) == 2:
        B = np.ascontiguousarray(B[:b[0], :b[1]])
    elif b is not None:
        B = no.synth_descriptors(b[0], b[1], planted=0.3, seed=b[2])[1]
    A.setflags(write=False); B.setflags(write=False)
    return A, B, S


@functools.lru_cache(maxsize=None)
def loop_reference(name, max_iter):
    """(xy1, xy2, notyet, unclear) per seed from the float64 oracle."""
    A, B, S = loop_scene(name)
    out = no.fast_reciprocal_NNs(A, B, S=S, max_iter=max_iter, dtype=np.float64, return_state=True)
    for a in out:
        a.setflags(write=False)
    return out
