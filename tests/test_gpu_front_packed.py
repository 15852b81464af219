"""Parity of the packed form of the banded tile sort (k_isect_emit_b's one-word store, k_rs_hist_band at shift 24,
k_rs_pass<BAND, PACKED>, k_band_offsets) on the cases of front_packed_cases.py: the sorted pair ids (peek 0) and the tile
offsets (peek 1) are the SAME BITS as the two-array form leaves (debug flag 1024) and as the oracle's lists, and so are the
images, the loss and the gradients; which form a step took is read from the emitted stream (peek 12): packed words carry the
low key byte above bit 24, the two-array form leaves bare pair ids there.
EXACT integers everywhere, so there is no error to report.

Measured on MI355X: 15 cases, 1.1 s after start-up; the slowest 0.7 s (the first step of the file), the two scenes of 2^21
Gaussians under 0.1 s each.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import front_band_cases as bcs
import front_packed_cases as pcs
import test_gpu_front as tf

DEV = tf.DEV
FLAG = pcs.FLAG_TWO_ARRAYS


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context(DEV)


def emitted(ctx, n):
    from starst3r_amd import ops
    return ops.peek(ctx, 12, n).clone().to(torch.int64) & 0xFFFFFFFF if n else torch.zeros(0, dtype=torch.int64, device=DEV)


def assert_stream(words, off, flat, n_keys, packed, label):
    """the emitted stream of a step against its sorted lists: the same multiset of (key, pair id) records.  Packed: the band
    of a word follows from its position (the band starts are the offsets of the keys b * 256), its low key byte sits above
    bit 24 and the pair id below; two arrays: the words are the bare pair ids."""
    n = int(flat.numel())
    assert words.numel() == n
    if n == 0:
        return
    counts = (off[1:] - off[:-1]).to(torch.int64)
    keys = torch.repeat_interleave(torch.arange(n_keys, device=DEV, dtype=torch.int64), counts)
    want = torch.sort((keys << pcs.PAIR_BITS) | flat.to(torch.int64)).values
    if not packed:
        assert torch.equal(torch.sort(words).values, torch.sort(flat.to(torch.int64)).values), (label, "bare pair ids")
        return
    starts = off[0:n_keys:256].to(torch.int64).contiguous()
    band = torch.searchsorted(starts, torch.arange(n, device=DEV, dtype=torch.int64), right=True) - 1
    got = (((band << 8) | (words >> pcs.PAIR_BITS)) << pcs.PAIR_BITS) | (words & ((1 << pcs.PAIR_BITS) - 1))
    assert torch.equal(torch.sort(got).values, want), (label, "packed words")
    if bool((keys & 0xFF).any()):
        assert bool((words >> pcs.PAIR_BITS).any())


# ---- 1. record cases: packed against two arrays against the oracle ----
@pytest.mark.parametrize("name", list(pcs.RECORD_CASES) + pcs.BANDED_CASES)
def test_raster_train_packed_vs_two_arrays_vs_oracle(ctx, name):
    from starst3r_amd import ops
    case = pcs.get(name)
    L = case.lists()
    assert pcs.packs(case) and bcs.plan(case)["banded"] == 1
    n_keys, n_px = case.Cn * case.n_tiles, case.Cn * case.H * case.W
    rec = tf.record_tensor(case)
    gt = torch.full((case.Cn, case.H, case.W, 3), 0.4, device=DEV)
    flat, off = tf.dev(L["flat"], torch.int32), tf.dev(L["off"], torch.int32)
    scan_ = tf.expected_scan(case.n_pairs, case.live_pid, L["tpg"])
    res = {}
    for flag in (0, FLAG):
        v, loss, n, lists = tf.raster_train(ctx, case, rec, gt, flag)
        assert n == L["n"]
        tf.assert_lists(lists, flat, off, scan_, (name, flag))
        assert_stream(emitted(ctx, n), off, flat, n_keys, flag == 0, (name, flag))
        res[flag] = (v, loss, ops.peek(ctx, 8, 3 * n_px, torch.float32).clone(), ops.peek(ctx, 9, n_px, torch.float32).clone())
    for a, b, what in zip(res[0], res[FLAG], ("gradients", "loss", "rgb", "alpha")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, what)
    assert bool(torch.isfinite(res[0][1]).all())
    if name == "no_record":
        assert not bool(lists[1].any())
    else:
        assert bool(torch.isfinite(res[0][0]).all())


def test_train_fwd_bwd_and_render_same_bits_in_both_forms(ctx):
    from starst3r_amd import ops
    case = pcs.get("banded_train"); R = case.reference()
    P, vm, K = tf.scene_tensors(case)
    campos = ops.camera_positions(vm)
    n, n_keys, n_px = R["n"], case.C * case.n_tiles, case.C * case.H * case.W
    want = tf.expected_scene_lists(case, R)
    img = {}
    for flag in (0, FLAG):
        ops.set_debug(ctx, flag)
        try:
            rgb, alpha, st = ops.render(ctx, P, vm, K, campos, case.W, case.H)
            torch.cuda.synchronize()
        finally:
            ops.set_debug(ctx, 0)
        assert st["n_isects"] == n
        tf.assert_lists(tf.fused_lists(ctx, n, n_keys, case.n_pairs), *want, ("render", flag))
        assert_stream(emitted(ctx, n), want[1], want[0], n_keys, flag == 0, ("render", flag))
        img[flag] = (rgb, alpha)
    assert torch.equal(img[0][0].view(torch.int32), img[FLAG][0].view(torch.int32))
    assert torch.equal(img[0][1].view(torch.int32), img[FLAG][1].view(torch.int32))
    gen = torch.Generator(device=DEV).manual_seed(12)
    gt = torch.clamp(img[0][0] + 0.1 * torch.randn(img[0][0].shape, device=DEV, generator=gen), 0, 1).contiguous()
    out = {}
    for flag in (0, FLAG):      # (the training call emits the tight rectangles: its lists are compared between the forms)
        g, l, st = tf.train(ctx, case, P, vm, K, campos, gt, flag)
        nt = st["n_isects"]
        assert 0 < nt <= n
        lists = tf.fused_lists(ctx, nt, n_keys, case.n_pairs)
        assert_stream(emitted(ctx, nt), lists[1], lists[0], n_keys, flag == 0, ("train", flag))
        out[flag] = (g, l, ops.peek(ctx, 8, 3 * n_px, torch.float32).clone(), ops.peek(ctx, 9, n_px, torch.float32).clone()) + lists
        assert bool(torch.isfinite(g).all())
    for a, b in zip(out[0], out[FLAG]):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    off = out[0][5]
    assert int(off[-1]) == nt and bool((off[1:] >= off[:-1]).all())


# ---- 2. the width of the pair id ----
def wide_step(ctx, case, P, vm, K, campos, gt, flag, call):
    from starst3r_amd import ops
    n_keys = case.C * case.n_tiles
    if call == "render":
        ops.set_debug(ctx, flag)
        try:
            rgb, alpha, st = ops.render(ctx, P, vm, K, campos, case.W, case.H)
            torch.cuda.synchronize()
        finally:
            ops.set_debug(ctx, 0)
        res = (rgb.reshape(-1), alpha.reshape(-1))
    else:
        g, l, st = tf.train(ctx, case, P, vm, K, campos, gt, flag)
        res = (g, l)
    n = st["n_isects"]
    flat, off, _ = tf.fused_lists(ctx, n, n_keys, case.n_pairs)
    return n, flat, off, res


@pytest.mark.parametrize("extra", [0, 1])
def test_pair_ids_of_24_bits_and_one_slot_more(extra):
    """N * C = 2^24: the packed form, and the pair id 0xFFFFFF comes back whole next to every key byte; N * C = 2^24 + C: the
    two arrays, with or without the flag.  The render call's lists are the oracle's; the training call (tight rectangles)
    is compared between the forms."""
    from starst3r_amd import ops
    case = pcs.get("wide_%d" % extra); R = case.reference()
    assert pcs.packs(case) == (extra == 0)
    P, vm, K = tf.scene_tensors(case)
    campos = ops.camera_positions(vm)
    gt = torch.full((case.C, case.H, case.W, 3), 0.4, device=DEV)
    n_keys = case.C * case.n_tiles
    want_flat, want_off = tf.dev(R["flat"], torch.int32), tf.dev(R["off"], torch.int32)
    top = case.n_pairs - 1
    ctx2 = ops.Context(DEV)
    try:
        for call in ("render", "train"):
            got = {}
            for flag in (0, FLAG):
                n, flat, off, res = wide_step(ctx2, case, P, vm, K, campos, gt, flag, call)
                if call == "render":
                    assert n == R["n"]
                    assert torch.equal(off, want_off) and torch.equal(flat, want_flat), (call, flag)
                assert_stream(emitted(ctx2, n), off, flat, n_keys, flag == 0 and extra == 0, (call, flag))
                assert int(flat.max()) == top and int(flat.min()) == 0 and bool((flat == top - 1).any())
                got[flag] = (flat, off) + res
            for a, b in zip(got[0], got[FLAG]):
                assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), call
    finally:
        ctx2.close()


# ---- 3. edge counts ----
def test_overflowing_step_same_lists_below_the_capacity_in_both_forms():
    """Debug flag 8 halves the capacity of an asynchronous step: records past it are dropped by the emission, the band table
    is clamped, and both forms must leave the same offsets (all of them: the clamped band starts, the closing count = the
    capacity) and the same sorted pair ids below the capacity -- and the next settle is loud."""
    from starst3r_amd import _lib, ops
    case = pcs.get("banded_train")
    P, vm, K = tf.scene_tensors(case)
    campos = ops.camera_positions(vm)
    gt = torch.full((case.C, case.H, case.W, 3), 0.4, device=DEV)
    n_keys = case.C * case.n_tiles
    got = {}
    for flag in (0, FLAG):
        ctx2 = ops.Context(DEV)
        try:
            g, l, st = tf.train(ctx2, case, P, vm, K, campos, gt, flag, want_stats=True)
            nt = st["n_isects"]; cap = nt // 2
            whole = tf.fused_lists(ctx2, nt, n_keys, case.n_pairs)
            tf.train(ctx2, case, P, vm, K, campos, gt, flag, want_stats=False)                 # leaves the sizing hint
            ops.settle(ctx2)
            tf.train(ctx2, case, P, vm, K, campos, gt, flag | 8, want_stats=False)
            off = ops.peek(ctx2, 1, n_keys + 1).clone(); flat = ops.peek(ctx2, 0, cap).clone()
            words = emitted(ctx2, cap)
            with pytest.raises(_lib.St3rError) as e:
                ops.settle(ctx2)
            assert "more than" in str(e.value)
            assert int(off[-1]) == cap and int(off.max()) == cap and bool((off[1:] >= off[:-1]).all())
            assert_stream(words, off, flat, n_keys, flag == 0, ("overflow", flag))
            # a band that ends below the capacity is complete: the whole step's list
            starts = whole[1].cpu().numpy().astype(np.int64)[0:n_keys:256]
            fits = int(max([0] + [e for e in np.append(starts[1:], nt).tolist() if e <= cap]))
            assert 0 < fits <= cap and torch.equal(flat[:fits], whole[0][:fits])
            got[flag] = (off, flat, whole[0], whole[1])
        finally:
            ctx2.close()
    for a, b, what in zip(got[0], got[FLAG], ("offsets", "pair ids below the capacity", "whole list", "whole offsets")):
        assert torch.equal(a, b), what
