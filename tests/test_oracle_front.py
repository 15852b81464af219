"""CPU pins of tests/front_cases.py -- the inputs of test_gpu_front.py -- with the oracle and the library's host-side plan
alone (no GPU): every planted property (rectangles, per-workgroup totals and first-output positions, chunks without a mark,
depth-code spans and pass counts, tie groups, n % 4, empty-key runs), the paths each case was written for (st3r_front_plan:
the decisions of rasterize_front and its callees, computed by the code that takes them), and the condition that lets the GPU
test demand the FULL oracle list: for every live pair of every case the restated tight_tile_rect (blend_cases.tile_rects,
shared with test_oracle_blend.py) equals the reference rectangle, so the fused path may leave out nothing -- the cap on
omitted (record, tile) pairs is zero."""
import numpy as np
import pytest

import blend_cases as bc
import front_cases as fc


def test_restated_constants_are_the_librarys():
    p = fc.plan(1000, 2, 64, 48)
    for name in fc.PLAN_CONSTANTS.values():
        assert p[name] == getattr(fc, name), name
    assert fc.LOOKBACK == 256          # chain_lookback256: one status word per thread of the 256-thread scan workgroup
    import ctypes
    from starst3r_amd import _lib
    out = (ctypes.c_int64 * 32)()
    L = _lib.lib()
    assert L.st3r_front_plan(0, 1, 16, 16, 0, 0, 0, 0, out, 32) != 0 and L.st3r_front_plan(1, 1, 16, 16, 0, 1, 1, 0, out, 32) != 0
    assert L.st3r_front_plan(1, 1, 16, 16, 0, 0, 0, 0, out, 31) != 0 and L.st3r_front_plan(1, 1, 16, 16, 0, 0, 0, 0, None, 32) != 0


def key_runs(case):
    """(occupied keys, longest run of empty keys in front, in the middle, behind)"""
    off = case.lists()["off"].astype(np.int64)
    occ = np.nonzero(np.diff(off) > 0)[0]
    total = case.Cn * case.n_tiles
    mid = int(np.diff(occ).max() - 1) if occ.size > 1 else 0
    return occ, (int(occ[0]), mid, int(total - 1 - occ[-1]))


def starts(tpg):
    return np.cumsum([0] + list(tpg))[:-1]


def marked_chunks(tpg):
    """per emission chunk of a workgroup: does a pair with tiles start in it?"""
    tpg = np.asarray(tpg)
    st = starts(tpg)[tpg > 0]
    total = int(tpg.sum())
    return [bool(((st >= c0) & (st < c0 + fc.ECH)).any()) for c0 in range(0, total, fc.ECH)]


# measured with the oracle (deterministic, CPU): records n, n % 4, live rows, occupied (camera, tile) keys
RECORD_PINS = {
    "scan_rects_4095": (4457, 1, 3199, 6), "scan_rects_4096": (3515, 3, 2559, 6), "scan_rects_4097": (5527, 3, 3864, 6),
    "emit_totals": (67266, 2, 20480, 72), "emit_big": (24765, 1, 16, 12240), "emit_widths": (2000, 0, 112, 136),
    "emit_strip_255x3": (4608, 0, 12, 765), "emit_strip_3x255": (4608, 0, 12, 765), "emit_strip_257x3": (4644, 0, 12, 771),
    "emit_cams_8_1000": (3435, 3, 5789, 42), "emit_cams_8_2049": (6596, 0, 10907, 42),
    "emit_cams_16_1000": (6558, 2, 10884, 84), "emit_cams_16_2049": (13321, 1, 22095, 84),
    "emit_cams_3_1025": (1545, 1, 2467, 18), "emit_cams_9_2047": (7562, 2, 12412, 48),
    "offs_keys_1": (7, 3, 7, 1), "offs_keys_2": (8, 0, 8, 2), "offs_keys_255": (9, 1, 9, 3), "offs_keys_256": (6, 2, 6, 3),
    "offs_keys_257": (7, 3, 7, 3),
    "offs_first_0": (3, 3, 3, 1), "offs_last_1": (4, 0, 4, 1), "offs_second_0": (160, 0, 160, 160),
    "offs_second_1": (161, 1, 161, 160), "offs_second_2": (162, 2, 162, 160), "offs_second_3": (163, 3, 163, 160),
    "offs_gap_2": (8, 0, 8, 2), "offs_runs_3": (486, 2, 486, 161),
    "keys_65552": (3, 3, 3, 3), "wg_scan": (35, 3, 10, 19),
}


@pytest.mark.parametrize("name", list(fc.RECORD_CASES))
def test_record_case_is_what_it_was_built_for(name, oracle_built):
    case = fc.get(name)
    L = case.lists()
    # the zero-omission condition: tight == reference for every live pair, so n_isects == n_isects_ref
    ref, tight = case.rects()
    assert np.array_equal(ref, tight), name
    area = (ref[:, 1] - ref[:, 0]) * (ref[:, 3] - ref[:, 2])
    assert np.array_equal(area, L["tpg"]) and int(area.sum()) == L["n"]
    # every live record is of the flat kind, its depth a code inside the 29-bit level-1 range, unique pair ids
    r = case.live_rows
    assert (r[:, 2] == 0.5).all() and (r[:, 3:6] == np.array(bc.FLAT_CONIC, np.float32)).all()
    assert (case.dbits() >= fc.NEAR_BITS).all() and (case.dbits() <= fc.FAR_BITS).all()
    occ, _ = key_runs(case)
    assert (L["n"], L["n"] % 4, case.live_pid.size, occ.size) == RECORD_PINS[name]
    # sorted keys ascending, offsets their run boundaries
    assert np.all(np.diff(L["keys"]) >= 0) and L["off"][-1] == L["n"]
    p = fc.plan(case.N, case.Cn, case.W, case.H, entry="records", n_records=L["n"])
    assert p["segments"] == 0 and p["key32"] == (case.Cn <= 8) and p["rectbase"] == 1
    assert p["rect32"] == (case.tw <= 255 and case.th <= 255)
    assert fc.plan(case.N, case.Cn, case.W, case.H, 64, "records")["rect32"] == 0
    assert fc.plan(case.N, case.Cn, case.W, case.H, 64, "records")["rectbase"] == 0


def test_planted_emission_edges(oracle_built):
    """by construction, not by measurement"""
    E = fc.ECH
    c = fc.get("emit_totals")
    wg0 = c.workgroups(0)
    assert [sum(w) for w in wg0] == fc.EMIT_TOTALS + [E - 1 + 6 + 3, E + 6 + 2, 1]
    assert [len(w) for w in wg0] == [fc.EP] * 8 + [1]                       # a last workgroup of ONE pair
    assert fc.EMIT_TOTALS == [0, 1, 4095, 4096, 4097, 12288]
    # a pair whose first output is output 0 / 4095 (last entry of chunk 0) / 4096 (first entry of chunk 1) of its workgroup
    assert wg0[2][0] > 0
    st6, st7 = starts(wg0[6]), starts(wg0[7])
    i6 = int(np.nonzero((st6 == E - 1) & (np.array(wg0[6]) > 0))[0][0])
    i7 = int(np.nonzero((st7 == E) & (np.array(wg0[7]) > 0))[0][0])
    assert wg0[6][i6] == 6 and st6[i6] == E - 1 and wg0[6][i6 + 1:i6 + 4] == [1, 1, 1]
    assert wg0[7][i7] == 6 and st7[i7] == E
    # the workgroup of 3 x 4096: chunk boundaries fall inside pairs (24 does not divide 4096): the carry crosses them
    assert all(t == 24 for t in wg0[5][:512]) and E % 24 != 0
    # all-empty workgroups between live ones; workgroups whose last pairs are all empty
    assert sum(wg0[0]) == 0 and sum(wg0[1]) == 1 and all(t == 0 for t in wg0[1][1:])
    wg1 = c.workgroups(1)
    assert [sum(w) for w in wg1] == ([sum(w) for w in wg0[:8]])[::-1] and len(wg1) == 8      # pair 8192 of camera 1 is culled
    wg2 = c.workgroups(2)
    assert np.nonzero(wg2[0])[0].tolist() == fc.LIVE_AT == [0, 255, 256, 1023]
    assert sum(wg2[1]) == 0 and np.nonzero(wg2[2])[0].tolist() == list(range(24)) and len(wg2[3]) == 1023
    assert fc.plan(c.N, c.Cn, c.W, c.H, entry="records")["bpc"] == 9 and c.Cn % 8 != 0            # the plain camera map

    b = fc.get("emit_big")
    (w,) = b.workgroups(0)
    assert w == [1, 4097, 1, 1, 1, 12240, 1, 1, 1, 1, 1, 8415, 1, 1, 1, 1]
    assert starts(w)[1] == 1 and w[1] == E + 1                               # 4097 tiles from output 1
    assert marked_chunks(w) == [True, True, False, True, False, False, True]   # chunks 2, 4 and 5 hold no mark
    ref, _ = b.rects()
    wh = {(int(r[1] - r[0]), int(r[3] - r[2])) for r in ref}
    assert {(241, 17), (255, 48), (255, 33), (1, 1)} == wh and (b.tw, b.th) == (255, 48)

    ref, _ = fc.get("emit_widths").rects()
    wh = {(int(r[1] - r[0]), int(r[3] - r[2])) for r in ref}
    assert wh == {(w_, h_) for w_ in fc.WIDTHS for h_ in (1, 2, 3, 4)} and fc.WIDTHS == [1, 2, 3, 5, 7, 15, 17]
    x0 = {int(r[0]) for r in ref}
    assert 0 in x0 and len(x0) > 5                                           # from the left edge and from the right one
    for name, (gw, gh), r32 in (("emit_strip_255x3", (255, 3), 1), ("emit_strip_3x255", (3, 255), 1),
                                ("emit_strip_257x3", (257, 3), 0)):
        s = fc.get(name)
        ref, _ = s.rects()
        wh = {(int(r[1] - r[0]), int(r[3] - r[2])) for r in ref}
        assert (s.tw, s.th) == (gw, gh) and {(gw, 1), (gw, gh), (gw - 1, gh), (1, gh)} <= wh
        p = fc.plan(s.N, s.Cn, s.W, s.H, entry="records")
        assert p["rect32"] == r32 and p["rectbase"] == 1
    # workgroup-to-camera maps: interleaved for 8 / 16 views with one and three workgroups per camera, plain for 3 / 9
    for name, C, bpc, last in (("emit_cams_8_1000", 8, 1, 1000), ("emit_cams_8_2049", 8, 3, 1), ("emit_cams_16_1000", 16, 1, 1000),
                               ("emit_cams_16_2049", 16, 3, 1), ("emit_cams_3_1025", 3, 2, 1), ("emit_cams_9_2047", 9, 2, 1023)):
        s = fc.get(name)
        p = fc.plan(s.N, s.Cn, s.W, s.H, entry="records")
        assert (s.Cn, p["bpc"], p["emit_grid"], p["self_base"]) == (C, bpc, C * bpc, 1) and s.N - (bpc - 1) * fc.EP == last
        per_cam = np.bincount(s.cams()[s.lists()["tpg"] > 0], minlength=C)
        assert (C < 8 or per_cam[7] == 0) and len(set(per_cam.tolist())) >= min(C, 6) - 1
        if C > 3:   # camera 3 has every pair visible: its last (ragged) workgroup is not empty of pairs
            assert per_cam[3] > 0 and np.count_nonzero(s.cams() == 3) == s.N


def test_planted_scan_sort_and_offset_edges(oracle_built):
    for n, tiles in ((4095, 1), (4096, 1), (4097, 2)):
        c = fc.get("scan_rects_%d" % n)
        assert c.n_pairs == n and fc.plan(c.N, c.Cn, c.W, c.H, entry="records")["scan_tiles"] == tiles
    # end_bit of the tile sort: C * tiles = 1, 2, 255, 256, 257 -> 0 (sorted as 1), 1, 8, 8, 9 bits
    for total, bits in ((1, 1), (2, 1), (255, 8), (256, 8), (257, 9)):
        c = fc.get("offs_keys_%d" % total)
        p = fc.plan(c.N, c.Cn, c.W, c.H, entry="records", n_records=c.lists()["n"])
        occ, _ = key_runs(c)
        assert c.Cn * c.n_tiles == total and p["end_bit"] == bits and p["ts_passes"] == (bits + 7) // 8
        assert occ[0] == 0 and occ[-1] == total - 1
    assert [fc.get("offs_second_%d" % e).lists()["n"] % 4 for e in range(4)] == [0, 1, 2, 3]
    assert key_runs(fc.get("offs_first_0")) [0].tolist() == [0] and key_runs(fc.get("offs_last_1"))[0].tolist() == [319]
    assert key_runs(fc.get("offs_second_0"))[0].tolist() == list(range(1, 320, 2))
    occ, runs = key_runs(fc.get("offs_gap_2"))
    assert occ.tolist() == [7, 308] and runs == (7, 300, 11)            # 300 empty keys between two occupied ones
    assert key_runs(fc.get("offs_runs_3"))[1] == (9, 100, 50)            # empty runs in front, in the middle and behind
    k = fc.get("keys_65552")
    p = fc.plan(k.N, k.Cn, k.W, k.H, entry="records", n_records=3)
    assert k.Cn * k.n_tiles == 65552 and p["end_bit"] == 17 and p["ts_passes"] == 3 and p["key32"] == 0
    assert key_runs(k)[0].tolist() == [0, 8 * 4097 + 8 * 241 + 120, 65551]
    # the emission takes its base from k_isect_wg_scan
    w = fc.get("wg_scan")
    p = fc.plan(w.N, w.Cn, w.W, w.H, entry="records", n_records=w.lists()["n"])
    assert (p["bpc"], p["emit_grid"], p["self_base"]) == (2050, 16400, 0) and p["emit_grid"] > fc.EMIT_SELF_BASE_MAX
    assert p["l1_small"] == 0 and p["scan_tiles"] > 2 * fc.LOOKBACK
    # every row is visible and all depth codes tie, so the level-1 order is the pair-id order and workgroup = index // EP
    assert w.fill is not None and (w.dbits() == fc.BASE).all() and w.fill[9:10].view(np.uint32)[0] == fc.BASE
    assert w.fill[10:11].view(np.int32)[0] > 0
    wgs = sorted({(int(pid // w.N), int(pid % w.N) // fc.EP) for pid in w.live_pid})
    assert wgs == [(0, 0), (0, 2048), (3, 1000), (5, 0), (7, 0), (7, 2049)]
    assert 8 * 2048 + 0 == fc.EMIT_SELF_BASE_MAX                         # (camera 0, workgroup 2048) is workgroup 16 384 of the launch
    assert w.N - 2049 * fc.EP == 1                                       # the last workgroup of a camera holds one pair
    # the thresholds themselves, on both sides (host arithmetic: no case has to be that large)
    P = lambda N, C, W, H, **kw: fc.plan(N, C, W, H, entry="records", **kw)
    assert [P(5, 1, 16 * t, 16)["rect32"] for t in (255, 256)] == [1, 0] == [P(5, 1, 16, 16 * t)["rect32"] for t in (255, 256)]
    assert [P(5, 1, 16 * t, 16)["rectbase"] for t in (1023, 1024)] == [1, 0] == [P(5, 1, 16, 16 * t)["rectbase"] for t in (1023, 1024)]
    assert [P(5, C, 16, 16)["key32"] for C in (8, 9)] == [1, 0]
    assert [P(2 * fc.EP, C, 16, 16)["self_base"] for C in (fc.EMIT_SELF_BASE_MAX // 2 // 64, 1)] == [1, 1]
    assert [P(fc.EP * g, 8, 16, 16)["self_base"] for g in (2048, 2049)] == [1, 0]
    assert [P(n, 1, 16, 16)["l1_small"] for n in (99 * fc.SORT_TILE_L32, 99 * fc.SORT_TILE_L32 + 1)] == [1, 0]
    assert [P(5, 1, 16, 16, n_records=n)["ts_small"] for n in (99 * fc.SORT_TILE_L32, 99 * fc.SORT_TILE_L32 + 1)] == [1, 0]
    assert [P(5, 1, 16 * t, 16)["end_bit"] for t in (1, 2, 3, 4, 5, 256, 257)] == [1, 1, 2, 2, 3, 8, 9]
    assert P(5, 8, 16, 16)["l1_passes"] == 4 and P(5, 9, 16, 16)["l1_passes"] == 5 and P(5, 1, 16, 16)["l1_passes"] == 4
    # stand-alone scan: tiles 1, 1, 1, 2, then 256, 256, 257 (one trip), 258 (two), 514 (three look-back trips at most)
    tiles = [fc.plan(n, 1, 16, 16, entry="records")["scan_tiles"] for n in fc.SCAN_SIZES]
    assert tiles == [1, 1, 1, 2, 256, 256, 257, 258, 514]
    assert [-(-(t - 1) // fc.LOOKBACK) for t in tiles[4:]] == [1, 1, 1, 2, 3]
    for n in fc.SCAN_SIZES:
        a = fc.scan_counts(n)
        assert a.max(initial=0) < 1 << 20 and (n < 100 or (a == 0).mean() > 0.25) and int(a.sum(dtype=np.int64)) < 2 ** 31
    for total in (2 ** 31 - 1, 2 ** 31):
        a = fc.scan_big_total(total)
        assert int(a.sum(dtype=np.int64)) == total and a.max() < 1 << 20 and np.count_nonzero(a) == 2049 and a.size > 2 * fc.SCAN_TILE


# live depth-code span, passes, views, N, Gaussians culled.  The level-1 product is the whole of span x N x (every Gaussian
# live | every third one culled: the indices 1, 4, 7, ...); the view count rotates over 1, 2, 7, 8 along it
SPAN_VALUES = [0, 254, 255, 256, 65534, 65535, 65536, 2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24, fc.FAR_BITS - fc.NEAR_BITS]
SPAN_PASSES = [1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]        # top = span + 1 at top < 2^8 / 2^16 / 2^24
NS = [4095, 4096, 4097, 8193]
third = lambda n: (n + 1) // 3                            # indices i % 3 == 1 below n
SCENE_PINS = {}
for i, s_ in enumerate(fc.SPANS):
    for j, n_ in enumerate(NS):
        for k in (0, 1):
            SCENE_PINS["span_%s_n%d%s" % (s_, n_, "_culled" * k)] = (SPAN_VALUES[i], SPAN_PASSES[i], [1, 2, 7, 8][(i + j + k) % 4],
                                                                    n_, third(n_) * k)
for n_ in NS:
    SCENE_PINS["nothing_n%d" % n_] = (None, 1, 2, n_, n_)
    for k in (0, 1):
        SCENE_PINS["blind_camera_n%d%s" % (n_, "_culled" * k)] = (256, 2, 3, n_, third(n_) * k)
SCENE_PINS.update({"views_9": (65536, 3, 9, 4097, 1366), "views_16": (255, 2, 16, 1000, 0), "ties": (None, 3, 2, 8193, 0),
                   "large": (None, 3, 8, 204803, 201803)})


def test_the_scene_list_is_the_product():
    assert sorted(SCENE_PINS) == sorted(fc.SCENE_CASES) and len(SCENE_PINS) == 11 * 4 * 2 + 4 + 8 + 4
    for i, s_ in enumerate(fc.SPANS):
        views = {SCENE_PINS["span_%s_n%d%s" % (s_, n_, "_culled" * k)][2] for n_ in NS for k in (0, 1)}
        assert views == {1, 2, 7, 8}
    # every pass count meets 1, 1, 2 and 3 small sort tiles per segment, with and without culled pairs
    seen = {(SPAN_PASSES[i], fc.plan(n_, 2, 48, 32)["tiles_per_seg"], k) for i in range(11) for n_ in NS for k in (0, 1)}
    assert seen == {(p_, t_, k) for p_ in (1, 2, 3, 4) for t_ in (1, 2, 3) for k in (0, 1)}


@pytest.mark.parametrize("name", list(fc.SCENE_CASES))
def test_scene_case_is_what_it_was_built_for(name, oracle_built):
    case = fc.get(name)
    R = case.reference(); m = R["meta"]
    span, passes, C, N, culled = SCENE_PINS[name]
    assert (case.C, case.N, case.N - case.live_idx.size) == (C, N, culled)
    # zero omission
    ref, tight = bc.tile_rects(m["means2d"], m["radii"], m["opacities"], m["conics"], case.tw, case.th)
    assert np.array_equal(ref, tight)
    assert int(((ref[:, 1] - ref[:, 0]) * (ref[:, 3] - ref[:, 2])).sum()) == R["n"] == int(m["tiles_per_gauss"].sum())
    # z = means[:, 2] exactly: the depth codes of the visible pairs are the planted bit patterns
    seen = np.zeros(0, np.uint32)
    if R["pid"].size:
        seen = m["depths"].view(np.uint32)
        assert np.array_equal(seen, case.zbits[np.searchsorted(case.live_idx, R["pid"] % case.N)])
        vis_cams = sorted(set(m["camera_ids"].tolist()))
        assert vis_cams == [c for c in range(C) if (not case.flip[c]) or (case.sign < 0).any()]
    if span is not None:
        assert int(seen.max()) - int(seen.min()) == span
    bias, top, np_ = R["krange"]
    assert np_ == passes and np_ == (1 if top < 256 else 2 if top < 65536 else 3 if top < 2 ** 24 else 4)
    if seen.size:
        assert bias == int(seen.min()) - fc.NEAR_BITS and top == int(seen.max()) - int(seen.min()) + 1
    else:
        assert (bias, top, np_) == (0, 1, 1)
    # the paths: training calls of up to 8 views sort camera segments of N pairs; more views: 64-bit keys, no segments;
    # render: 32-bit keys without segments; debug flag 4: no segments
    p = fc.plan(N, C, case.W, case.H, n_records=R["n"])
    assert p["key32"] == (C <= 8) and p["segments"] == (C <= 8) and p["rect32"] == 1 and p["rectbase"] == 1
    small = -(-C * N // fc.SORT_TILE_L32) < fc.RS_SMALL_BELOW
    assert p["l1_small"] == small
    if C <= 8:
        assert p["tiles_per_seg"] == -(-N // (fc.SORT_TILE_S32 if small else fc.SORT_TILE_L32))
        assert p["l1_tiles"] == p["tiles_per_seg"] * C
    else:
        assert p["tiles_per_seg"] == 0 and p["l1_tile"] == fc.SORT_TILE_S64
    assert fc.plan(N, C, case.W, case.H, 4)["segments"] == 0 and fc.plan(N, C, case.W, case.H, 64)["rect32"] == 0
    q = fc.plan(N, C, case.W, case.H, entry="render")
    assert q["segments"] == 0 and q["key32"] == (C <= 8)


def test_planted_key_and_tie_edges(oracle_built):
    """by construction"""
    assert fc.SPANS == [0, 254, 255, 256, 65534, 65535, 65536, 2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24, "near_far"]
    # k_reg_reduce: passes from the sentinel top = span + 1 at top < 2^8 / 2^16 / 2^24
    assert SPAN_PASSES == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4] and fc.SPAN_N == NS
    assert [fc.passes_for(fc.BASE, fc.BASE + s)[2] for s in fc.SPANS[:-1]] == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
    # N on both sides of one and two small sort tiles, every view count of the 32-bit keys, culled pairs interleaved
    # (the product itself: test_the_scene_list_is_the_product)
    assert {(n, fc.plan(n, 2, 48, 32)["tiles_per_seg"]) for n in fc.SPAN_N} == {(4095, 1), (4096, 1), (4097, 2), (8193, 3)}
    c = fc.get("span_254_n4096_culled")
    assert np.array_equal(c.live_idx, np.arange(c.N)[np.arange(c.N) % 3 != 1])
    nf = fc.get("span_near_far_n4097")
    assert fc.NEAR_BITS in nf.zbits and fc.FAR_BITS in nf.zbits             # z = 0.01 exactly together with z = 1e10 exactly
    assert nf.zbits.view(np.float32).min() == np.float32(0.01) and nf.zbits.view(np.float32).max() == np.float32(1e10)
    # ties: groups of 2, 3, 64, 65 and 4097 identical depth codes inside a camera, the same codes in the other camera
    t = fc.get("ties")
    vals, counts = np.unique(t.zbits, return_counts=True)
    assert sorted(counts[counts > 1].tolist()) == fc.TIE_GROUPS == [2, 3, 64, 65, 4097]
    big = t.live_idx[t.zbits == vals[np.argmax(counts)]]
    assert set((big // fc.SORT_TILE_S32).tolist()) == {0, 1, 2}             # spread over all three sort tiles of the segment
    assert t.C == 2 and not any(t.flip)
    # the tied pairs reach the same tiles: the oracle orders them by pair id inside every tile list
    R = t.reference()
    code = t.zbits[np.searchsorted(t.live_idx, R["flat"] % t.N)].astype(np.int64)
    key = np.repeat(np.arange(t.C * t.n_tiles), np.diff(R["off"]))
    same = (key[1:] == key[:-1]) & (code[1:] == code[:-1])
    assert same.sum() > 4000 and np.all(R["flat"][1:][same] > R["flat"][:-1][same])
    # one camera with every pair culled while the others see everything
    b = fc.get("blind_camera_n4097")
    assert b.flip == [False, True, False] and sorted(set(b.reference()["meta"]["camera_ids"].tolist())) == [0, 2]
    # the large scene: 400 whole scan tiles and a bit, two look-back trips; the segmented sort's large shape, 13 tiles per
    # segment with a ragged last one; planted Gaussians in the first, a middle and the last EP block of the indices
    g = fc.get("large")
    p = fc.plan(g.N, g.C, g.W, g.H, n_records=g.reference()["n"])
    assert g.n_pairs == 1638424 and p["scan_tiles"] == 401 and -(-(401 - 1) // fc.LOOKBACK) == 2
    assert (p["l1_small"], p["l1_tile"], p["tiles_per_seg"], p["l1_tiles"]) == (0, 16384, 13, 104) and g.N % 16384 != 0
    assert -(-g.n_pairs // fc.SORT_TILE_L32) == 101 >= fc.RS_SMALL_BELOW
    assert sorted(set((g.live_idx // fc.EP).tolist())) == [0, 100, 199, 200]
    assert sorted(set(g.reference()["meta"]["camera_ids"].tolist())) == list(range(8)) and (g.sign > 0).sum() > 1000 < (g.sign < 0).sum()
