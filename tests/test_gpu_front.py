"""Planted-edge parity of the fused front end (k_records_prepare / k_project_sh_fwd level-1 keys and rectangles,
k_scan_chained, k_isect_gather / k_isect_wg_scan / k_isect_emit_d, the segmented and device-count radix sorts,
k_isect_offsets32) and of the stage calls (k_isect_emit, k_isect_offsets) through the C ABI against oracle/gs_oracle.c, on
the hand-written cases of front_cases.py.  EXACT integers everywhere: the sorted pair-id list (peek 0) is the oracle's
(camera, tile, depth bits, pair id) order, the offsets (peek 1) its run boundaries plus the closing total, the pair scan
(peek 3) the cumulative rectangle areas, the statistics the counts.  Nothing may be left out: test_oracle_front.py holds, per
live pair of every case, that the tight rectangle of the fused path is the reference rectangle.

What each case plants, and the host-side paths it reaches (asserted there through st3r_front_plan): front_cases.py,
test_oracle_front.py.  `rectbase` cannot be peeked; the blend backward consumes it, so the gradients of every case must be
the same BITS with it (flag 0), without it (flag 64: 64-bit rectangles), with recomputed rectangles (flag 2, training calls)
and under the other blend forms (flags 128, 1) -- and equal to the stage path's bits, which takes the slot index from
reference rectangles.

Measured on MI355X: MEASURED at the end of this file.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import front_cases as fc

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops.get_context(DEV)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def scattered(n, idx, vals, dtype):
    """zeros(n) with vals written at idx, built on the device (no host array of n entries)"""
    out = torch.zeros((n,) + tuple(np.shape(vals)[1:]), dtype=dtype, device=DEV)
    if len(idx):
        out[dev(idx, torch.int64)] = dev(vals, dtype)
    return out


def record_tensor(case):
    rec = torch.zeros((case.n_pairs, 12), device=DEV)
    if case.fill is not None:
        rec[:] = dev(case.fill)
    rec[dev(case.live_pid, torch.int64)] = dev(case.live_rows)
    return rec


def expected_scan(n_pairs, pid, tpg):
    return torch.cumsum(scattered(n_pairs, pid, tpg, torch.int64), 0).to(torch.int32)


def fused_lists(ctx, n, n_keys, n_pairs):
    from starst3r_amd import ops
    flat = ops.peek(ctx, 0, n).clone() if n else torch.zeros(0, dtype=torch.int32, device=DEV)
    return flat, ops.peek(ctx, 1, n_keys + 1).clone(), ops.peek(ctx, 3, n_pairs).clone()


def assert_lists(got, flat, off, scan, label):
    g_flat, g_off, g_scan = got
    assert torch.equal(g_off, off), (label, "offsets")
    assert torch.equal(g_flat, flat), (label, "sorted pair ids")
    assert torch.equal(g_scan, scan), (label, "pair scan")


# ---- 1. the scan on its own ----
def scan(ctx, a):
    from starst3r_amd import ops
    cum, total = ops.isect_scan(ctx, dev(a, torch.int32))
    torch.cuda.synchronize()
    return cum.cpu().numpy().astype(np.int64), total


@pytest.mark.parametrize("n", fc.SCAN_SIZES)
def test_scan_vs_cumsum(ctx, n):
    a = fc.scan_counts(n)
    want = np.cumsum(a, dtype=np.int64)
    for _ in range(2):      # (a second launch meets the first one's status words: another generation)
        cum, total = scan(ctx, a)
        assert total == int(want[-1]) < 2 ** 31
        assert np.array_equal(cum, want)


def test_scan_of_zeros(ctx):
    n = (fc.LOOKBACK + 1) * fc.SCAN_TILE + 5
    cum, total = scan(ctx, np.zeros(n, np.int32))
    assert total == 0 and not cum.any()


def test_scan_total_at_the_int32_limit(ctx):
    """a grand total of 2^31 - 1 comes back as it is; 2^31 is reported by the kernel as -1, which st3r_gs_isect_scan turns
    into an error (include/st3r.h) instead of handing back a wrapped scan"""
    from starst3r_amd import ops
    a = fc.scan_big_total(2 ** 31 - 1)
    cum, total = scan(ctx, a)
    assert total == 2 ** 31 - 1 and np.array_equal(cum, np.cumsum(a, dtype=np.int64))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.isect_scan(ctx, dev(fc.scan_big_total(2 ** 31), torch.int32))
    cum, total = scan(ctx, a)                                  # the context is as good as before
    assert total == 2 ** 31 - 1


# ---- 2. record cases: the fused path behind st3r_gs_raster_train, and the stage calls ----
RECORD_FLAGS = {64: "64-bit packed rectangles, no rectbase", 2: "(recomputed rectangles: training calls only)",
                128: "quadrant TRAIN forward", 1: "no quadrant / cell culling"}


def raster_train(ctx, case, rec, gt, flag):
    from starst3r_amd import ops
    ops.set_debug(ctx, flag)
    try:
        v = torch.full((case.n_pairs, 12), float("nan"), device=DEV); loss = torch.zeros(1, device=DEV)
        st = ops.raster_train(ctx, rec, case.N, case.Cn, gt, case.W, case.H, 0.2, v, loss)
        torch.cuda.synchronize()
        return v, loss, st["n_isects"], fused_lists(ctx, st["n_isects"], case.Cn * case.n_tiles, case.n_pairs)
    finally:
        ops.set_debug(ctx, 0)


def stage_path(ctx, case, rec, gt):
    """ops.isect / sort_pairs / offsets against the oracle, then blend forward, loss and blend backward on those lists"""
    from starst3r_amd import ops
    L = case.lists()
    tiles = scattered(case.n_pairs, case.live_pid, L["tpg"], torch.int32)
    cum, ids, flat = ops.isect(ctx, rec, tiles, case.N, case.Cn, case.W, case.H)
    end_bit = 32 + case.n_tiles.bit_length() + case.Cn.bit_length()
    ids_s, flat_s = ops.sort_pairs(ctx, ids, flat, end_bit)
    off = ops.offsets(ctx, ids_s, case.Cn, case.W, case.H)
    torch.cuda.synchronize()
    assert torch.equal(cum, expected_scan(case.n_pairs, case.live_pid, L["tpg"]))
    assert torch.equal(ids, dev(L["ids_unsorted"], torch.int64)) and torch.equal(flat, dev(L["flat_unsorted"], torch.int32))
    assert torch.equal(ids_s, dev(L["ids"], torch.int64)) and torch.equal(flat_s, dev(L["flat"], torch.int32))
    assert torch.equal(off.reshape(-1), dev(L["off"][:-1], torch.int32))
    rgb, alpha, last = ops.blend_fwd(ctx, rec, off, flat_s, case.Cn, case.W, case.H)
    sums, v_rgb = ops.loss_l1_ssim(ctx, rgb, gt, 0.8, 0.2)
    v = ops.blend_bwd(ctx, rec, off, flat_s, alpha, last, v_rgb, None, cum, case.Cn, case.W, case.H)
    torch.cuda.synchronize()
    return v, rgb, alpha


@pytest.mark.parametrize("name", list(fc.RECORD_CASES))
def test_raster_train_lists_vs_oracle(ctx, name):
    from starst3r_amd import ops
    case = fc.get(name)
    L = case.lists()
    rec = record_tensor(case)
    gt = torch.full((case.Cn, case.H, case.W, 3), 0.4, device=DEV)
    flat, off = dev(L["flat"], torch.int32), dev(L["off"], torch.int32)
    scan_ = expected_scan(case.n_pairs, case.live_pid, L["tpg"])
    v0, loss0, n0, lists0 = raster_train(ctx, case, rec, gt, 0)
    assert n0 == L["n"]
    assert_lists(lists0, flat, off, scan_, name)
    n_px = case.Cn * case.H * case.W
    rgb0 = ops.peek(ctx, 8, 3 * n_px, torch.float32).clone(); alpha0 = ops.peek(ctx, 9, n_px, torch.float32).clone()
    assert bool(torch.isfinite(v0).all()) and bool(torch.isfinite(loss0).all())
    for flag, what in RECORD_FLAGS.items():
        v, loss, n, lists = raster_train(ctx, case, rec, gt, flag)
        assert n == n0, what
        assert_lists(lists, flat, off, scan_, (name, what))
        assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), what
        assert torch.equal(v.view(torch.int32), v0.view(torch.int32)), what
        del v
    # the stage calls on the same records (k_isect_emit, the 64-bit sort, k_isect_offsets), and their gradients: the slot index
    # from reference rectangles instead of rectbase -- the same slots, the same sums
    v_stage, rgb_s, alpha_s = stage_path(ctx, case, rec, gt)
    assert torch.equal(rgb0.view(torch.int32), rgb_s.reshape(-1).view(torch.int32))        # the images, bit for bit
    assert torch.equal(alpha0.view(torch.int32), alpha_s.reshape(-1).view(torch.int32))
    bad = int((v_stage.view(torch.int32) != v0.view(torch.int32)).sum())
    print("%s: %d records, %d of %d gradient words differ from the stage path" % (name, n0, bad, v0.numel()))
    assert bad == 0


# ---- 3. scene cases: st3r_gs_train_fwd_bwd (segmented level-1 sort), st3r_gs_render, the stage path ----
def scene_tensors(case):
    N = case.N
    g = case.live
    P = dict(means=scattered(N, case.live_idx, g["means"], torch.float32), quats=scattered(N, case.live_idx, g["quats"], torch.float32),
             scales=scattered(N, case.live_idx, g["scales"], torch.float32),
             opacities=scattered(N, case.live_idx, g["opacities"], torch.float32),
             shN=scattered(N, case.live_idx, g["shN"], torch.float32))
    P["quats"][:, 0] = 1.0          # the culled Gaussians: all zero (z = 0 < near) but for a unit quaternion
    return P, dev(case.viewmats), dev(case.Ks)


_stage = {}


def scene_stage(ctx, name):
    """tensors, the stage path's images and lists (asserted equal to the oracle's), a ground truth; shared, never modified"""
    if name in _stage:
        return _stage[name]
    from starst3r_amd import ops
    case = fc.get(name); R = case.reference()
    P, vm, K = scene_tensors(case)
    rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], vm, K, case.W, case.H)
    torch.cuda.synchronize()
    assert torch.equal(info["_flatten_ids_dense"], dev(R["flat"], torch.int32))
    assert torch.equal(info["isect_offsets"].reshape(-1), dev(R["off"][:-1], torch.int32))
    gen = torch.Generator(device=DEV).manual_seed(11)
    gt = torch.clamp(rgb + 0.1 * torch.randn(rgb.shape, device=DEV, generator=gen), 0, 1).contiguous()
    if len(_stage) >= 2:
        _stage.clear()              # (only the test that follows needs it: keep the device memory of two cases at most)
    _stage[name] = (case, R, P, vm, K, ops.camera_positions(vm), rgb, alpha, gt)
    return _stage[name]


def expected_scene_lists(case, R):
    return (dev(R["flat"], torch.int32), dev(R["off"], torch.int32),
            expected_scan(case.n_pairs, R["pid"], R["meta"]["tiles_per_gauss"]))


TRAIN_FLAGS = {4: "(camera | depth) level-1 keys, no segments", 64: "64-bit packed rectangles, no rectbase",
               2: "the backward recomputes the rectangles"}


def train(ctx, case, P, vm, K, campos, gt, flag, want_stats=True):
    from starst3r_amd import ops
    ops.set_debug(ctx, flag)
    try:
        grads = torch.full((23 * case.N,), float("nan"), device=DEV); loss = torch.zeros(1, device=DEV)
        st = ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, case.W, case.H, 0.2, 0.01, 0.01, grads, loss, want_stats=want_stats)
        torch.cuda.synchronize()
        return grads, loss, st
    finally:
        ops.set_debug(ctx, 0)


@pytest.mark.parametrize("name", list(fc.SCENE_CASES))
def test_train_fwd_bwd_lists_vs_oracle(ctx, name):
    from starst3r_amd import ops
    case, R, P, vm, K, campos, rgb, alpha, gt = scene_stage(ctx, name)
    n, n_keys = R["n"], case.C * case.n_tiles
    want = expected_scene_lists(case, R)
    g0, l0, st = train(ctx, case, P, vm, K, campos, gt, 0)
    assert (st["n_isects"], st["n_isects_ref"], st["n_visible"]) == (n, n, R["pid"].size)
    assert_lists(fused_lists(ctx, n, n_keys, case.n_pairs), *want, name)
    if case.C <= 8:
        # the level-1 sort by camera segments: bias, sentinel and the pass count the depth codes of the call need
        krange = tuple(ops.peek(ctx, 10, 16)[8:11].tolist())
        print("%s: bias, sentinel, passes = %s" % (name, krange))
        assert krange == R["krange"]
    for which, full in ((8, rgb), (9, alpha)):      # the stage path's images, bit for bit
        got = ops.peek(ctx, which, full.numel(), torch.float32)
        assert torch.equal(got.view(torch.int32), full.reshape(-1).view(torch.int32)), which
    # Gradients: finite wherever float32 can hold them.  The span_near_far scenes put Gaussians at z up to 1e10 with raw scales up to
    # 8e8 (sigma 8 px on the image), and the scale regulariser of the training loss is exp(scale): it overflows above
    # scale = 88.7, i.e. z = 1109 here (measured at N = 4097: 2350 of the Gaussians, z from 1.12e3 up) -- such a Gaussian's gradient
    # is not finite in any float32 evaluation, every other one must be
    bad = ~torch.isfinite(g0)
    if name.startswith("span_near_far"):
        rows = torch.zeros(case.N, dtype=torch.bool, device=DEV)
        for blk in ops.split_grads(bad, case.N).values():
            rows |= blk.reshape(case.N, -1).any(1)
        z = P["means"][:, 2]
        print("%s: %d of %d Gaussians have a non-finite gradient, their z from %.3g to %.3g"
              % (name, int(rows.sum()), case.N, float(z[rows].min()) if bool(rows.any()) else 0.0,
                 float(z[rows].max()) if bool(rows.any()) else 0.0))
        assert not bool(rows[P["scales"][:, 0] <= 88.0].any())
    else:
        assert not bool(bad.any())
    for flag, what in TRAIN_FLAGS.items():
        g, l, st2 = train(ctx, case, P, vm, K, campos, gt, flag)
        assert st2 == st, what
        assert_lists(fused_lists(ctx, n, n_keys, case.n_pairs), *want, (name, what))
        assert torch.equal(l.view(torch.int32), l0.view(torch.int32)), what
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32)), what
    # The record count on the device: capacity above the count, tickets past the last tile of the tile sort.  On a FRESH
    # context (no sizing hint of another scene with the same N, C, W, H) a call without statistics sizes itself exactly the
    # first time and leaves the hint; the next one does not synchronise.  That it took that path is read from control word 0
    # of the context, zeroed when allocated, which only the scan of an asynchronous step writes (the count, for k_adam).
    ctx2 = ops.Context(DEV)
    try:
        for call in range(2):
            g, l, none_ = train(ctx2, case, P, vm, K, campos, gt, 0, want_stats=False)
            assert none_ is None
            ops.settle(ctx2)
            word0 = int(ops.peek(ctx2, 10, 16)[0])
            # (nothing visible: no count to size from, so such a call never leaves the synchronous path)
            assert word0 == (n if call == 1 else 0), (name, call, word0)
            assert_lists(fused_lists(ctx2, n, n_keys, case.n_pairs), *want, (name, "call %d without statistics" % call))
            assert torch.equal(g.view(torch.int32), g0.view(torch.int32)) and torch.equal(l.view(torch.int32), l0.view(torch.int32))
    finally:
        ctx2.close()


@pytest.mark.parametrize("name", list(fc.SCENE_CASES))
def test_render_lists_vs_oracle(ctx, name):
    """st3r_gs_render: 32-bit level-1 keys WITHOUT segments up to 8 views (29 + camera bits), reference rectangles"""
    from starst3r_amd import ops
    case, R, P, vm, K, campos, rgb, alpha, gt = scene_stage(ctx, name)
    r, a, st = ops.render(ctx, P, vm, K, campos, case.W, case.H)
    torch.cuda.synchronize()
    assert st["n_isects"] == R["n"]
    assert_lists(fused_lists(ctx, R["n"], case.C * case.n_tiles, case.n_pairs), *expected_scene_lists(case, R), name)
    # the stage path's images, bit for bit
    assert torch.equal(r.view(torch.int32), rgb.view(torch.int32))
    assert torch.equal(a.reshape(-1).view(torch.int32), alpha.reshape(-1).view(torch.int32))


# MEASURED (MI355X): every comparison is exact, so there is no error to report; on every record case 0 gradient words differ
# from the stage path (201 424 992 words on `wg_scan`).  Run time: 249 cases, 7.6 s (9.3 s with start-up); the slowest case
# 0.6 s (the first training call of the file), the three device-built cases under 0.1 s each.
# Mutations (each run once against this file and against the older front-end tests), the mutants argued from the code
# instead of run, and the defect found (st3r_gs_isect_scan at a total of 2^31): DESIGN.md, "Front end on every scan, key,
# emission, sort and offset edge".
