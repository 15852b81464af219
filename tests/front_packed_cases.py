"""Hand-written inputs for the packed form of the banded tile sort (no torch, no GPU), next to front_band_cases.py, whose
cases and builders they use: with N * C <= 2^24 pair slots the banded emission writes ONE word per record, pair id | low
key byte << 24, the low-byte pass sorts that word keys-only and stores the bare pair ids, and the tile offsets come from the
band table and the band histograms (radix_sort.hip: k_rs_pass<PACKED>, k_band_offsets).  Debug flag 1024 keeps the two
arrays (tile keys next to pair ids, offsets read back from the sorted keys); both forms must leave the same bits.

Used by test_front_packed_cases.py (CPU: every case has the layout it is named for, from the oracle's sorted keys) and
test_gpu_front_packed.py (the kernels).
"""
import numpy as np

import front_band_cases as bcs
import front_cases as fc

FLAG_TWO_ARRAYS = 1024
PAIR_BITS = 24


def bins_0_255():
    """C = 2, 272 x 256 (17 x 16 = 272 tiles a camera, 544 keys, three bands): records on the keys 0 and 255 (band 0: bins 0
    and 255 and nothing between), 256 and 511 (band 1, the camera boundary 272 inside it) -- and none at all in band 2
    (keys 512 .. 543).  Another count on every key, the depths interleaved."""
    b = fc.Records("bins_0_255", 272, 256, 2, None, 41)
    left = {0: 37, 255: 64, 256: 65, 511: 130}
    while any(left.values()):
        for k in left:
            if left[k]:
                b.key(k); left[k] -= 1
    return b.build()


def hollow_ends():
    """C = 3, 400 x 304 (475 tiles a camera, 1425 keys, six bands): records on the keys 300 .. 1100 only -- the tiles 0 .. 299
    in front (all of band 0 among them) and 1101 .. 1424 behind (all of band 5) are empty, so the offsets start with 301
    zeros and end with 325 times the record count; every tenth key in between is empty as well."""
    b = fc.Records("hollow_ends", 400, 304, 3, 1500, 42)
    rng = np.random.default_rng(42)
    for k in range(300, 1101):
        if k % 10 != 4:
            b.key(k, int(rng.integers(1, 4)))
    return b.build()


def one_record():
    """C = 3, 400 x 304: one record in all, on key 700 (band 2, bin 188) -- five bands without a record around it"""
    return fc.Records("one_record", 400, 304, 3, 50, 43).key(700).build()


def no_record():
    """C = 3, 400 x 304: fifty tile-less records and culled pairs, not one record"""
    b = fc.Records("no_record", 400, 304, 3, 90, 44)
    for c in range(3):
        b.none(c, 50)
    return b.build()


RECORD_CASES = {"bins_0_255": bins_0_255, "hollow_ends": hollow_ends, "one_record": one_record, "no_record": no_record}
# the cases of front_band_cases.py that run in the packed form as well: a band without a record between two that have some,
# camera boundaries inside bands, runs of one key around a sort tile (the small shape), the large tile shape
BANDED_CASES = ["two_bands", "six_bands", "keys_272", "empty_band", "equal_runs", "empty_workgroup", "large_shape"]


WIDE_W = WIDE_H = 96        # 6 x 6 tiles a camera, 8 cameras: 288 keys, two bands


def wide_scene(extra):
    """C = 8, 96 x 96, N = 2^21 + extra Gaussians of which 400 are in front of the cameras -- the first and the last two
    indices among them, so the pair ids 0, N * C - 2 and N * C - 1 are live -- and every other one is behind them (all zero:
    z = 0).  extra = 0: N * C = 2^24 exactly, the largest pair id 0xFFFFFF fills all 24 bits under the key byte; extra = 1:
    2^24 + 8 pair slots, one too many for the packed word."""
    N = (1 << 21) + extra
    rng = np.random.default_rng(2024 + 45 + extra)
    idx = np.unique(np.concatenate([[0, 1, N - 2, N - 1], rng.integers(0, N, 396)]))
    zb = fc._span_bits(4096, idx.size, rng)
    px = rng.uniform(4, WIDE_W - 4, idx.size); py = rng.uniform(4, WIDE_H - 4, idx.size)
    for i in (0, 1, -2, -1):            # well inside every camera's image (the principal points differ by up to 21 pixels)
        px[i], py[i] = 40.0, 50.0
    return fc.SceneCase("wide_%d" % extra, WIDE_W, WIDE_H, N, idx, zb, np.ones(idx.size), px, py, [False] * 8, 45 + extra)


_cache = {}


def get(name):
    if name in BANDED_CASES or name == "banded_train":
        return bcs.get(name)
    if name not in _cache:
        _cache[name] = wide_scene(int(name[5:])) if name.startswith("wide_") else RECORD_CASES[name]()
    return _cache[name]


def packs(case):
    """does a step on this case take the packed form?"""
    Cn = case.Cn if hasattr(case, "Cn") else case.C
    n_keys = Cn * case.n_tiles
    return 256 < n_keys <= 65536 and case.N * Cn <= 1 << PAIR_BITS


def packed_pairs(keys, flat):
    """the multiset of records as sorted words key << 24 | pair id (int64)"""
    return np.sort((np.asarray(keys, np.int64) << PAIR_BITS) | np.asarray(flat, np.int64))
