"""Hand-written inputs for the banded form of the tile sort (no torch, no GPU), next to front_cases.py, whose builders
they use: the emission writes the records split by the high byte of their (camera, tile) key -- the band -- and one stable
low-byte pass per band is left of the level-2 sort (gs_isect.hip: k_isect_gather's band counts, k_band_table,
k_isect_emit_b; radix_sort.hip: k_rs_hist_band, k_rs_pass<BAND>).  The form applies to keys of 9 .. 16 bits; debug flag 16
keeps the plain emission and the two passes, and both must leave the same bits.

Used by test_oracle_front_banded.py (CPU: every case has the band layout it is named for, from the oracle's sorted keys,
and reaches the path it is meant to reach, through st3r_front_plan) and test_gpu_front_banded.py (the kernels).
"""
import numpy as np

import front_cases as fc

FLAG_TWO_PASS = 16
EP, ECH = fc.EP, fc.ECH
SORT_TILE_S = fc.SORT_TILE_S32        # every case but large_shape stays below RS_SMALL_BELOW large tiles: the small tile shape


def n_bands(case):
    return ((case.Cn * case.n_tiles - 1) >> 8) + 1


def band_lengths(case):
    """records per band, from the oracle's sorted (camera, tile) keys"""
    return np.bincount(np.asarray(case.lists()["keys"], np.int64) >> 8, minlength=n_bands(case))


def band_range(case, cam):
    """first and last band that hold keys of camera `cam`"""
    return (cam * case.n_tiles) >> 8, ((cam + 1) * case.n_tiles - 1) >> 8


def two_bands():
    """C = 2, 272 x 208 (17 x 13 = 221 tiles a camera, 442 keys): two bands, the camera boundary (key 221) inside band 0.
    N = 700: one ragged emission workgroup per camera, a random mix of rectangles, tile-less and culled pairs."""
    return fc._random_records("two_bands", 272, 208, 2, 700, 31)


def six_bands():
    """C = 3, 400 x 304 (25 x 19 = 475 tiles a camera, 1425 keys): six bands, cameras 0 | 1 meet inside band 1 and 1 | 2
    inside band 3, and since 256 is no multiple of 25 the band edges fall inside tile rows.  Every camera starts with 20
    Gaussians whose rectangle is the whole image (475 outputs each -- a pair cannot have more outputs than the image has
    tiles, so it is the WORKGROUP that has more than ECH outputs here: 9500 from these pairs, three chunks) and goes on with
    a random mix; N = EP + 300: a second, ragged workgroup per camera."""
    b = fc.Records("six_bands", 400, 304, 3, EP + 300, 32)
    rng = np.random.default_rng(32)
    for c in range(3):
        b.tl(c, b.tw, b.th, 20)
        for _ in range(EP + 200):
            u = rng.random()
            if u < 0.3:
                (b.tl if rng.random() < 0.5 else b.br)(c, int(rng.integers(1, b.tw + 1)), int(rng.integers(1, b.th + 1)))
            elif u < 0.5:
                b.none(c)
            else:
                b.one(c, int(rng.integers(0, b.tw)), int(rng.integers(0, b.th)))
    return b.build()


def keys_256():
    """C = 1, 256 x 256: exactly 256 keys, end_bit 8 -- one band, one pass anyway: the fallback"""
    return fc._random_records("keys_256", 256, 256, 1, 600, 33)


def keys_272():
    """C = 1, 272 x 256 (17 x 16): 272 keys, the second band holds the last 16 of them -- two records in all"""
    b = fc.Records("keys_272", 272, 256, 1, 500, 34)
    rng = np.random.default_rng(34)
    for _ in range(400):
        b.one(0, int(rng.integers(0, 17)), int(rng.integers(0, 15)))      # keys 0 .. 254
    b.key(255).key(256).key(271)
    return b.build()


def empty_band():
    """C = 3, 400 x 304: every Gaussian in the top tile rows -- camera 0 in rows 0 and 1 (keys 0 .. 49: band 0), cameras 1 and
    2 in row 0 (keys 475 .. 499: band 1; 950 .. 974: band 3): bands 2, 4 and 5 are empty, band 2 between two that are not"""
    b = fc.Records("empty_band", 400, 304, 3, 300, 35)
    rng = np.random.default_rng(35)
    for c in range(3):
        for _ in range(250):
            b.one(c, int(rng.integers(0, 25)), int(rng.integers(0, 2 if c == 0 else 1)))
        b.tl(c, 25, 2 if c == 0 else 1, 3)
    return b.build()


RUN_KEYS = {3: SORT_TILE_S - 1, 200: SORT_TILE_S, 271: SORT_TILE_S + 1}


def equal_runs():
    """C = 1, 272 x 256: TILE - 1, TILE and TILE + 1 single-tile Gaussians of distinct depths stacked on the keys 3, 200
    (band 0) and 271 (band 1), TILE = 4096, the small sort tile: runs of one low byte that end one short of a sort tile, on
    it and one past it -- and, all depths distinct, the order inside a run is the depth order alone (stability).  The three
    stacks are interleaved in depth, so every emission workgroup feeds all three runs."""
    b = fc.Records("equal_runs", 272, 256, 1, None, 36)
    left = dict(RUN_KEYS)
    while any(left.values()):
        for k in RUN_KEYS:
            if left[k]:
                b.key(k); left[k] -= 1
    return b.build()


def empty_workgroup():
    """C = 2, 272 x 208, N = 2 EP + 5 (no multiple of EP): the middle workgroup of camera 0 and the first one of camera 1
    hold tile-less records only, the last workgroup of either camera five pairs"""
    b = fc.Records("empty_workgroup", 272, 208, 2, 2 * EP + 5, 37, shuffle=True)
    rng = np.random.default_rng(37)

    def live(c, n):
        for _ in range(n):
            if rng.random() < 0.2:
                (b.tl if rng.random() < 0.5 else b.br)(c, int(rng.integers(1, 18)), int(rng.integers(1, 14)))
            else:
                b.one(c, int(rng.integers(0, 17)), int(rng.integers(0, 13)))
    live(0, EP); b.none(0, EP); live(0, 5)
    b.none(1, EP); live(1, EP); live(1, 5)
    return b.build()


def large_shape():
    """C = 3, 400 x 304, N = 1200: per camera 1170 Gaussians whose rectangle is the whole image (475 outputs each) among 30
    single tiles -- 1 667 280 records, just above RS_SMALL_BELOW = 100 large sort tiles (1 638 400): the 1024-thread,
    16 384-item tile shape of the banded pass that the flagship workload runs, about 17 tiles per band, the last one ragged"""
    b = fc.Records("large_shape", 400, 304, 3, 1200, 38)
    rng = np.random.default_rng(38)
    for c in range(3):
        for i in range(1200):
            if i % 40 == 7:
                b.one(c, int(rng.integers(0, b.tw)), int(rng.integers(0, b.th)))
            else:
                b.tl(c, b.tw, b.th)
    return b.build()


RECORD_CASES = {"large_shape": large_shape, "two_bands": two_bands, "six_bands": six_bands, "keys_256": keys_256, "keys_272": keys_272,
                "empty_band": empty_band, "equal_runs": equal_runs, "empty_workgroup": empty_workgroup}


def train_scene():
    """C = 3, 400 x 304, N = 3000 Gaussians under the identity cameras (front_cases.SceneCase), every third one culled: the
    six-band shape for st3r_gs_train_fwd_bwd / st3r_gs_render, synchronous and asynchronous"""
    return fc._scene("banded_train", 3000, [False] * 3, lambda L, rng: fc._span_bits(65536, L, rng), 71, culled_every=3,
                     W=400, H=304)


_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = train_scene() if name == "banded_train" else RECORD_CASES[name]()
    return _cache[name]


def plan(case, flags=0, entry="records", n_records=0):
    """front_cases.plan plus the words of the banded form: taken, bands, launch tiles of its pass"""
    import ctypes
    from starst3r_amd import _lib
    Cn = case.Cn if hasattr(case, "Cn") else case.C
    out = (ctypes.c_int64 * 32)()
    _lib.check(_lib.lib().st3r_front_plan(case.N, Cn, case.W, case.H, flags, int(entry == "train"), int(entry == "records"),
                                          n_records, out, 32))
    d = fc.plan(case.N, Cn, case.W, case.H, flags, entry, n_records)
    d.update(banded=int(out[18]), bands=int(out[19]), band_tiles=int(out[30]))
    return d
