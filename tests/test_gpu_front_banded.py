"""Parity of the banded tile sort (k_isect_gather's band counts, k_band_table, k_isect_emit_b, k_rs_hist_band,
k_rs_pass<BAND>) on the cases of front_band_cases.py: for every case the offsets and the sorted pair ids are the SAME BITS as
the plain emission + two-pass sort leave (debug flag 16) and as the oracle's lists; one training call gives the same loss,
images and gradients on both paths; the asynchronous device-count path and its loud overflow keep working, nothing is
written past the capacity, and a wrap of either scan's status-word generation leaves the record count alone.
EXACT integers everywhere, so there is no error to report.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import front_band_cases as bcs
import front_cases as fc
import test_gpu_front as tf

DEV = tf.DEV
FLAG = bcs.FLAG_TWO_PASS


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context(DEV)


@pytest.mark.parametrize("name", list(bcs.RECORD_CASES))
def test_raster_train_lists_banded_vs_two_pass_vs_oracle(ctx, name):
    case = bcs.get(name)
    L = case.lists()
    assert bcs.plan(case)["banded"] == (0 if name == "keys_256" else 1)
    rec = tf.record_tensor(case)
    gt = torch.full((case.Cn, case.H, case.W, 3), 0.4, device=DEV)
    flat, off = tf.dev(L["flat"], torch.int32), tf.dev(L["off"], torch.int32)
    scan_ = tf.expected_scan(case.n_pairs, case.live_pid, L["tpg"])
    v0, loss0, n0, lists0 = tf.raster_train(ctx, case, rec, gt, 0)
    assert n0 == L["n"]
    tf.assert_lists(lists0, flat, off, scan_, (name, "banded"))
    v1, loss1, n1, lists1 = tf.raster_train(ctx, case, rec, gt, FLAG)
    assert n1 == n0
    tf.assert_lists(lists1, flat, off, scan_, (name, "two passes"))
    assert torch.equal(loss0.view(torch.int32), loss1.view(torch.int32))
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    if name == "equal_runs":   # stability, spelled out: inside a run of one key the pair ids follow the depth order
        order = case.live_pid[case.depth_order(0)]
        keys = np.asarray(L["keys"], np.int64)
        got = lists0[0].cpu().numpy()
        r = case.live_rows[case.depth_order(0)]
        k_of = (r[:, 1] // 16).astype(np.int64) * case.tw + (r[:, 0] // 16).astype(np.int64)
        for k in bcs.RUN_KEYS:
            assert np.array_equal(got[keys == k], order[k_of == k]), k


def test_train_fwd_bwd_and_render_same_bits_on_both_paths(ctx):
    from starst3r_amd import ops
    case = bcs.get("banded_train"); R = case.reference()
    P, vm, K = tf.scene_tensors(case)
    campos = ops.camera_positions(vm)
    n, n_keys = R["n"], case.C * case.n_tiles
    want = tf.expected_scene_lists(case, R)
    rgb, alpha, st = ops.render(ctx, P, vm, K, campos, case.W, case.H)
    torch.cuda.synchronize()
    assert st["n_isects"] == n
    tf.assert_lists(tf.fused_lists(ctx, n, n_keys, case.n_pairs), *want, "render, banded")
    gen = torch.Generator(device=DEV).manual_seed(12)
    gt = torch.clamp(rgb + 0.1 * torch.randn(rgb.shape, device=DEV, generator=gen), 0, 1).contiguous()
    # (the training call emits the TIGHT rectangles: fewer records than the oracle's reference rectangles on an image of this
    # size, so its lists are compared between the two paths, the render call's above against the oracle)
    out, lists = {}, {}
    for flag in (0, FLAG):
        g, l, st = tf.train(ctx, case, P, vm, K, campos, gt, flag)
        nt = st["n_isects"]
        assert 0 < nt <= n and st["n_isects_ref"] == n
        lists[flag] = tf.fused_lists(ctx, nt, n_keys, case.n_pairs)
        n_px = case.C * case.H * case.W
        out[flag] = (g, l, ops.peek(ctx, 8, 3 * n_px, torch.float32).clone(), ops.peek(ctx, 9, n_px, torch.float32).clone())
        assert bool(torch.isfinite(g).all())
    for a, b in zip(out[0] + lists[0], out[FLAG] + lists[FLAG]):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    want_t, nt = lists[0], int(lists[0][0].numel())
    assert int(want_t[1][-1]) == nt and bool((want_t[1][1:] >= want_t[1][:-1]).all())
    ops.set_debug(ctx, FLAG)
    try:
        r2, a2, _ = ops.render(ctx, P, vm, K, campos, case.W, case.H)
        torch.cuda.synchronize()
    finally:
        ops.set_debug(ctx, 0)
    assert torch.equal(r2.view(torch.int32), rgb.view(torch.int32)) and torch.equal(a2.view(torch.int32), alpha.view(torch.int32))
    assert torch.equal(out[0][2], rgb.reshape(-1))       # the training call renders the same image

    # two consecutive calls without statistics on a fresh context: the second keeps the count on the device (control word
    # 0 of the context is written by the scan of an asynchronous step only); then the test hook halves the capacity of an
    # asynchronous step: records past it are dropped, the bands below the capacity are still sorted, the next call is loud
    ctx2 = ops.Context(DEV)
    try:
        for call in range(2):
            g, l, none_ = tf.train(ctx2, case, P, vm, K, campos, gt, 0, want_stats=False)
            assert none_ is None
            ops.settle(ctx2)
            assert int(ops.peek(ctx2, 10, 16)[0]) == (nt if call == 1 else 0)
            tf.assert_lists(tf.fused_lists(ctx2, nt, n_keys, case.n_pairs), *want_t, ("asynchronous", call))
            assert torch.equal(g.view(torch.int32), out[0][0].view(torch.int32)) and torch.equal(l, out[0][1])
        from starst3r_amd import _lib
        g, l, none_ = tf.train(ctx2, case, P, vm, K, campos, gt, 8, want_stats=False)
        cap = nt // 2
        off = want_t[1].cpu().numpy().astype(np.int64)
        starts = off[0:n_keys:256]                          # first position of every band
        whole = int(max([0] + [e for e in np.append(starts[1:], nt).tolist() if e <= cap]))
        assert 0 < whole <= cap
        flat = ops.peek(ctx2, 0, cap).clone()
        assert torch.equal(flat[:whole], want_t[0][:whole])   # every band that fits below the capacity: complete and sorted
        with pytest.raises(_lib.St3rError) as e:
            ops.settle(ctx2)
        assert "more than" in str(e.value)
        g, l, _ = tf.train(ctx2, case, P, vm, K, campos, gt, 0, want_stats=False)     # recovered (synchronous)
        tf.assert_lists(tf.fused_lists(ctx2, nt, n_keys, case.n_pairs), *want_t, "after the overflow")
        assert torch.equal(g.view(torch.int32), out[0][0].view(torch.int32))
    finally:
        ctx2.close()


@pytest.mark.parametrize("ahead", [0, 1])
def test_generation_wrap_of_either_scan_keeps_the_record_count(ahead):
    """A step runs two single-pass scans, the pair-order scan, whose total IS the record count every later kernel reads
    from device memory, and the band-counter scan behind it.  When the 14-bit generation of a scan's status words runs out,
    its control block -- which holds the total -- is cleared in stream order.  Debug flag 256 puts both generations two or
    three launches before their end; `ahead` more stand-alone scans move the pair-order scan's wrap one step forward, so that
    over the five steps either scan wraps with the other one's total live.  Every step must leave the oracle's lists."""
    from starst3r_amd import ops
    case = bcs.get("six_bands")
    L = case.lists()
    rec = tf.record_tensor(case)
    gt = torch.full((case.Cn, case.H, case.W, 3), 0.4, device=DEV)
    want = (tf.dev(L["flat"], torch.int32), tf.dev(L["off"], torch.int32), tf.expected_scan(case.n_pairs, case.live_pid, L["tpg"]))
    ctx2 = ops.Context(DEV)
    try:
        v0, loss0, n0, lists0 = tf.raster_train(ctx2, case, rec, gt, 0)      # sizes every buffer
        tf.assert_lists(lists0, *want, "first step")
        ops.set_debug(ctx2, 256); ops.set_debug(ctx2, 0)
        for _ in range(ahead):
            ops.isect_scan(ctx2, tf.dev(np.arange(5000) % 7, torch.int32))
        for step in range(5):
            v, loss, n, lists = tf.raster_train(ctx2, case, rec, gt, 0)
            assert n == L["n"]
            tf.assert_lists(lists, *want, ("step after the hook", step))
            assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(loss, loss0)
    finally:
        ctx2.close()


def test_overflowing_step_leaves_everything_past_the_capacity_alone():
    """The guard region: a fresh context sizes the emitted and the sorted key / pair-id arrays for exactly the nt records of
    its first step.  The next step runs on the same Gaussians in REVERSED order (other pair ids in every record, the same
    count) with the capacity halved by debug flag 8: all four arrays must keep the first step's contents from the capacity
    on -- and must have changed below it, or the comparison would prove nothing."""
    from starst3r_amd import _lib, ops
    case = bcs.get("banded_train")
    P, vm, K = tf.scene_tensors(case)
    campos = ops.camera_positions(vm)
    gt = torch.full((case.C, case.H, case.W, 3), 0.4, device=DEV)
    Pr = {k: torch.flip(v, [0]).contiguous() for k, v in P.items()}
    ctx3 = ops.Context(DEV)
    try:
        g, l, st = tf.train(ctx3, case, P, vm, K, campos, gt, 0, want_stats=True)
        nt = st["n_isects"]; cap = nt // 2
        tf.train(ctx3, case, P, vm, K, campos, gt, 0, want_stats=False)                     # leaves the sizing hint
        ops.settle(ctx3)
        which = {11: "emitted keys", 12: "emitted pair ids", 13: "sorted keys", 0: "sorted pair ids"}
        before = {w: ops.peek(ctx3, w, nt).clone() for w in which}
        tf.train(ctx3, case, Pr, vm, K, campos, gt, 8, want_stats=False)
        for w, what in which.items():
            after = ops.peek(ctx3, w, nt)
            assert torch.equal(after[cap:], before[w][cap:]), what
        assert not torch.equal(ops.peek(ctx3, 12, nt)[:cap], before[12][:cap])
        assert not torch.equal(ops.peek(ctx3, 0, nt)[:cap], before[0][:cap])
        with pytest.raises(_lib.St3rError) as e:
            ops.settle(ctx3)
        assert "more than" in str(e.value)
    finally:
        ctx3.close()
