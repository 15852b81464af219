"""CPU pins of front_band_cases.py: every case has the band layout it is named for (from the oracle's sorted keys) and
reaches the path it was written for (st3r_front_plan: host arithmetic, no GPU)."""
import numpy as np

import front_band_cases as bcs
import front_cases as fc


def cam_bands(case):
    keys = np.asarray(case.lists()["keys"], np.int64)
    return [set((keys[keys // case.n_tiles == c] >> 8).tolist()) for c in range(case.Cn)]


def test_plan_words_of_the_banded_form():
    case = bcs.get("six_bands")
    n = case.lists()["n"]
    p, q = bcs.plan(case, 0, n_records=n), bcs.plan(case, bcs.FLAG_TWO_PASS, n_records=n)
    assert (p["banded"], p["bands"], q["banded"], q["bands"], q["band_tiles"]) == (1, 6, 0, 0, 0)
    assert p["band_tiles"] == n // p["ts_tile"] + 6
    # every word that described the call before keeps its value, with and without the banded form
    for k in fc.PLAN_FIELDS + tuple(fc.PLAN_CONSTANTS.values()):
        assert p[k] == q[k] == fc.plan(case.N, case.Cn, case.W, case.H, 0, "records", n)[k], k
    assert (p["end_bit"], p["ts_passes"], p["ts_small"], p["ts_tile"]) == (11, 2, 1, fc.SORT_TILE_S32)
    # the range of the form: keys of 9 .. 16 bits, every entry
    for entry in ("train", "records", "render"):
        assert fc.plan(100, 1, 256, 256, entry=entry)["end_bit"] == 8 and bcs.plan(bcs.get("keys_256"), entry=entry)["banded"] == 0
        assert bcs.plan(bcs.get("keys_272"), entry=entry)["banded"] == 1
    big = fc.get("keys_65552")
    assert bcs.plan(big)["banded"] == 0 and fc.plan(big.N, big.Cn, big.W, big.H, entry="records")["end_bit"] == 17
    flagship = fc.plan(1_000_000, 8, 1920, 1080, n_records=26_000_000)
    assert (flagship["end_bit"], flagship["ts_passes"], flagship["ts_small"]) == (16, 2, 0)
    import ctypes
    from starst3r_amd import _lib
    out = (ctypes.c_int64 * 32)()
    _lib.check(_lib.lib().st3r_front_plan(1_000_000, 8, 1920, 1080, 0, 1, 0, 26_000_000, out, 32))
    assert (out[18], out[19], out[30]) == (1, 255, 26_000_000 // fc.SORT_TILE_L32 + 255)


def test_two_bands_camera_boundary_inside_a_band():
    case = bcs.get("two_bands")
    assert (case.n_tiles, bcs.n_bands(case)) == (221, 2) and bcs.plan(case)["banded"] == 1
    cb = cam_bands(case)
    assert cb[0] == {0} and cb[1] == {0, 1} and (bcs.band_lengths(case) > 0).all()
    assert bcs.band_range(case, 0) == (0, 0) and bcs.band_range(case, 1) == (0, 1)
    assert case.N % fc.EP != 0 and bcs.plan(case)["bpc"] == 1


def test_six_bands_edges_inside_tile_rows_and_chunks():
    case = bcs.get("six_bands")
    assert (case.n_tiles, bcs.n_bands(case)) == (475, 6) and (bcs.band_lengths(case) > 0).all()
    cb = cam_bands(case)
    assert cb[0] == {0, 1} and cb[1] == {1, 2, 3} and cb[2] == {3, 4, 5}
    for c in range(3):
        wgs = case.workgroups(c)
        assert len(wgs) == 2 and sum(wgs[0]) > 2 * fc.ECH and wgs[0][:20] == [475] * 20
        # a band edge inside a tile row of this camera: some multiple of 256 is no row start
        assert any((e - c * 475) % 25 for e in range(256, 1425, 256) if c * 475 < e < (c + 1) * 475)


def test_around_256_keys():
    a, b = bcs.get("keys_256"), bcs.get("keys_272")
    assert a.n_tiles == 256 and bcs.plan(a)["end_bit"] == 8 and bcs.plan(a)["banded"] == 0 and a.lists()["n"] > 0
    assert b.n_tiles == 272 and bcs.plan(b)["end_bit"] == 9 and bcs.plan(b)["banded"] == 1
    assert bcs.band_lengths(b).tolist() == [401, 2]


def test_empty_band_between_two_that_are_not():
    case = bcs.get("empty_band")
    L = bcs.band_lengths(case)
    assert L[0] > 0 and L[1] > 0 and L[2] == 0 and L[3] > 0 and L[4] == 0 and L[5] == 0


def test_equal_runs_around_a_sort_tile():
    case = bcs.get("equal_runs")
    keys = np.asarray(case.lists()["keys"], np.int64)
    assert {int(k): int((keys == k).sum()) for k in np.unique(keys)} == bcs.RUN_KEYS
    p = bcs.plan(case, n_records=keys.size)
    assert (p["banded"], p["ts_small"], p["ts_tile"]) == (1, 1, bcs.SORT_TILE_S) and np.unique(case.dbits()).size == keys.size
    assert bcs.band_lengths(case).tolist() == [2 * bcs.SORT_TILE_S - 1, bcs.SORT_TILE_S + 1]
    # every emission workgroup but the ragged last feeds all three runs
    order = case.depth_order(0)
    r = case.live_rows[order]
    k = (r[:, 1] // 16).astype(np.int64) * 17 + (r[:, 0] // 16).astype(np.int64)
    assert all(set(k[i:i + fc.EP].tolist()) == set(bcs.RUN_KEYS) for i in range(0, 11 * fc.EP, fc.EP))


def test_empty_workgroups_and_ragged_n():
    case = bcs.get("empty_workgroup")
    assert case.N % fc.EP == 5 and bcs.plan(case)["bpc"] == 3
    w0, w1 = case.workgroups(0), case.workgroups(1)
    assert [sum(w) > 0 for w in w0] == [True, False, True] and [sum(w) > 0 for w in w1] == [False, True, True]
    assert len(w0[2]) == 5 and len(w1[2]) == 5


def test_train_scene_has_six_live_bands():
    s = bcs.get("banded_train")
    R = s.reference()
    off = R["off"].astype(np.int64)
    per_key = np.diff(off)
    L = np.add.reduceat(per_key, np.arange(0, per_key.size, 256))
    assert L.size == 6 and (L > 0).all() and int(L.sum()) == R["n"]
    assert bcs.plan(s, entry="train")["banded"] == 1 and bcs.plan(s, entry="render")["banded"] == 1


def test_large_shape_reaches_the_large_sort_tile():
    case = bcs.get("large_shape")
    n = case.lists()["n"]
    p = bcs.plan(case, n_records=n)
    assert n == 3 * (1170 * 475 + 30) and n > fc.RS_SMALL_BELOW * fc.SORT_TILE_L32
    assert (p["banded"], p["bands"], p["ts_small"], p["ts_tile"]) == (1, 6, 0, fc.SORT_TILE_L32)
    L = bcs.band_lengths(case)
    assert (L > 2 * fc.SORT_TILE_L32).all() and (L % fc.SORT_TILE_L32 != 0).all()      # several tiles a band, the last ragged
