"""CPU: every case of front_packed_cases.py has the layout it is named for, read from the oracle's sorted (camera, tile)
keys, and reaches the form of the tile sort it is meant to reach (st3r_front_plan for the banded form, the pair-slot rule
for the packed word)."""
import numpy as np
import pytest

import front_band_cases as bcs
import front_packed_cases as pcs


def band_hist(case):
    keys = np.asarray(case.lists()["keys"], np.int64)
    return np.bincount(keys, minlength=bcs.n_bands(case) * 256).reshape(-1, 256)


def test_bins_0_255():
    case = pcs.get("bins_0_255")
    h = band_hist(case)
    assert h.shape[0] == 3 and case.n_tiles % 256 != 0 and 256 < case.n_tiles < 512    # the camera boundary inside band 1
    assert h[0].nonzero()[0].tolist() == [0, 255] and h[1].nonzero()[0].tolist() == [0, 255] and not h[2].any()
    assert len({int(h[0, 0]), int(h[0, 255]), int(h[1, 0]), int(h[1, 255])}) == 4


def test_hollow_ends():
    case = pcs.get("hollow_ends")
    L = case.lists()
    keys, off = np.asarray(L["keys"], np.int64), np.asarray(L["off"], np.int64)
    assert keys.min() == 300 and keys.max() == 1100 and not np.isin(keys, np.arange(304, 1100, 10)).any()
    h = band_hist(case)
    assert h.shape[0] == 6 and not h[0].any() and not h[5].any() and all(h[b].any() for b in (1, 2, 3, 4))
    assert not off[:301].any() and (off[1101:] == L["n"]).all() and off.size == 1426
    assert case.n_tiles % 256 != 0


def test_edge_counts():
    one, none_ = pcs.get("one_record"), pcs.get("no_record")
    assert one.lists()["n"] == 1 and np.asarray(one.lists()["keys"]).tolist() == [700]
    assert none_.lists()["n"] == 0 and none_.live_pid.size == 150


@pytest.mark.parametrize("name", list(pcs.RECORD_CASES) + pcs.BANDED_CASES + ["banded_train"])
def test_cases_take_the_packed_banded_form(name):
    case = pcs.get(name)
    assert pcs.packs(case)
    entry = "train" if name == "banded_train" else "records"
    assert bcs.plan(case, 0, entry)["banded"] == 1 and bcs.plan(case, pcs.FLAG_TWO_ARRAYS, entry)["banded"] == 1
    assert bcs.plan(case, bcs.FLAG_TWO_PASS, entry)["banded"] == 0


def test_longer_than_a_sort_tile():
    assert bcs.get("equal_runs").lists()["n"] > 2 * bcs.SORT_TILE_S         # the small tile shape, three tiles
    assert max(bcs.RUN_KEYS.values()) > bcs.SORT_TILE_S                     # one RUN of a key longer than a tile


def test_wide_scenes_sit_on_either_side_of_the_pair_id_width():
    at, past = pcs.get("wide_0"), pcs.get("wide_1")
    assert at.n_pairs == 1 << 24 and pcs.packs(at) and bcs.plan(at, 0, "train")["banded"] == 1
    assert past.n_pairs == (1 << 24) + past.C and not pcs.packs(past) and bcs.plan(past, 0, "train")["banded"] == 1
    for case in (at, past):
        R = case.reference()
        flat = np.asarray(R["flat"], np.int64)
        assert 0 < R["n"] < 100000 and flat.max() == case.n_pairs - 1 and flat.min() == 0
        assert np.isin([case.n_pairs - 2, 7 * case.N], flat).all()
        assert (np.diff(R["off"][::256]) > 0).all()                          # both bands hold records
