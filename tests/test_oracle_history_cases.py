"""CPU pins of tests/history_cases.py, from the oracle alone: every condition that a planted history of
test_gpu_history.py relies on holds with a factor of at least 1.5 to its threshold.  (The GPU file asserts the same facts
once more from the calls' own statistics.)"""
import pytest

import history_cases as hc

ROOM = 1.5


@pytest.fixture(scope="module")
def counts():
    got = {name: hc.records(name) for name in hc.RECORDS}
    assert got == hc.RECORDS          # the pinned counts that test_gpu_history.py compares the calls' statistics with
    return got


def test_record_counts_lie_on_the_intended_side_of_the_touch_threshold(counts):
    """st3r_blend_bwd_impl marks touched pairs once a call keeps more than 8 records per pair slot (n > 8 N C)"""
    for name, n in counts.items():
        N, V = hc.SCENES[name][:2]
        print("%s: %d records, %.2f of 8 N C = %d" % (name, n, n / (8 * N * V), 8 * N * V))
        if hc.TOUCH[name]:
            assert n >= ROOM * 8 * N * V, (name, n)
        else:
            assert n * ROOM <= 8 * N * V, (name, n)


def test_the_two_seeds_of_a_scene_share_a_shape_and_do_not_grow_the_arena(counts):
    """same (N, C, W, H): the same hint signature, the same per-pair buffers; and the second seed's records fit what the
    first one's left (+25 %), whichever comes first"""
    for a, b in hc.PAIRS:
        assert hc.SCENES[a][:4] == hc.SCENES[b][:4] and hc.SCENES[a][4] != hc.SCENES[b][4]
        na, nb = counts[a], counts[b]
        # 40-byte colour slots: no growth (the counts differ by a few per cent; the headroom is 25 %: a factor of 1.5 on the
        # DIFFERENCE), nor an asynchronous overflow
        assert min(na, nb) + ROOM * abs(na - nb) <= hc.GROW(40 * min(na, nb)) // 40, (a, b, na, nb)
        assert min(na, nb) + ROOM * abs(na - nb) <= min(na, nb) + min(na, nb) // 4 + 1024


def test_dense_small_outgrows_every_capacity_a_large_call_leaves(counts):
    """a synchronous `large` call leaves slots for n + 25 %; an asynchronous one is given hint + 25 % + 1024 records and the
    arena adds its own 25 % on top.  dense_small needs 1.5 x more than either, at no more than 8 records per pair / 1.5."""
    big = max(counts["large/a"], counts["large/b"])
    cap_sync = hc.GROW(40 * big) // 40
    cap_async = hc.GROW(40 * (big + big // 4 + 1024)) // 40
    n = counts["dense_small"]
    print("dense_small %d records; a large call leaves room for %d (synchronous) / %d (asynchronous)" % (n, cap_sync, cap_async))
    assert n >= ROOM * cap_async and cap_async >= cap_sync
    N, V = hc.SCENES["dense_small"][:2]
    assert n * ROOM <= 8 * N * V
    # (no planted condition, it only fixes which calls grow the slots -- large -> dense_small -> regular, nothing fits the
    # other way round; the GPU file asserts every growth it names from arena_bytes)
    assert min(counts["regular/a"], counts["regular/b"]) > hc.GROW(40 * n) // 40


@pytest.mark.parametrize("a,b", hc.PAIRS)
def test_each_seed_reads_slots_that_only_the_other_seed_writes(a, b):
    """at least a tenth (x 1.5) of a seed's slot-owning pairs own a slot that the other seed's backward writes and its own
    does not: a gather that took a stale stamp for a live one would add it"""
    for mine, other in ((a, b), (b, a)):
        f = hc.stale_pairs(mine, other)
        print("%s after %s: %.3f of the pairs read a slot only the other wrote" % (mine, other, f))
        assert f >= ROOM * 0.1, (mine, other, f)


def test_catalogue_is_well_formed():
    for name, c in hc.CALLS.items():
        assert c.name == name and c.kind in ("train", "other") and (c.kind == "other" or c.views >= 1)
    assert set(hc.SHUFFLE) == set(hc.CALLS)
    assert {"radix_sort:%d" % n for n in (hc.SORT_TILE - 1, hc.SORT_TILE + 1)} <= set(hc.CALLS)
