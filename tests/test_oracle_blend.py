"""CPU pins of tests/blend_cases.py -- the inputs of test_gpu_blend.py -- with the oracle alone (no GPU):
the per-tile list depths every case was built for, the planted saturation indices, the depths the fused path's exact
culling must keep, and the oracle's clear fraction (margin > 1e-4: the share of pixels whose skip / stop decisions float32
determines).  The clear fraction is 1.0 for EVERY case, the needle conics included: test_gpu_blend.py masks nothing."""
import numpy as np
import pytest

import blend_cases as bc


def measure(name):
    case = bc.get(name); R = bc.reference(name)
    _, _, flat, off = case.lists()
    o = np.append(off.reshape(-1), flat.shape[0])
    last, sat = [], []
    for c in range(case.Cn):
        for ty in range(case.th):
            for tx in range(case.tw):
                t = (c * case.th + ty) * case.tw + tx
                sl = (c, slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
                # last blended record, local to the tile's list, over the pixels that blended something ([-1, -1]: none did;
                # the oracle leaves last_ids = 0 there, whatever the tile's start)
                touched = R["fwd"]["alpha"][sl][..., 0] > 0
                u = R["fwd"]["last"][sl][touched] - o[t]
                last.append([int(u.min()), int(u.max())] if u.size else [-1, -1])
                assert not R["fwd"]["last"][sl][~touched].any()
                # a pixel whose loop stopped: something behind its last blended record would still pass the alpha test
                # (float64 evaluation: T_final <= 2e-4 and the list goes on)
                sat.append(int((1.0 - R["f64"]["alpha"][sl] <= 2.5e-4).sum()))
    m = R["fwd"]["margin"]
    return dict(depths=case.tile_depths(), kept=bc.fused_kept_depths(case) if name in bc.FUSED else None, last=last,
                saturated=sat, clear=float((m > 1e-4).mean()), min_margin=float(m.min()))


# measured with the oracle (deterministic, CPU); per tile in (view, tile row, tile column) order
PINS = {
    'depth_v9': dict(depths=[0, 1, 3, 4, 5, 63, 64, 65, 0],
        kept=None,
        last=[[-1, -1], [0, 0], [1, 1], [3, 3], [3, 3], [60, 60], [63, 63], [63, 63], [-1, -1]],
        saturated=[0, 0, 0, 0, 0, 0, 0, 0, 0], clear=1.0, min_margin=1.000),
    'depth_v8': dict(depths=[255, 256, 257, 0, 511, 512, 513, 769],
        kept=None,
        last=[[252, 252], [255, 255], [255, 255], [-1, -1], [510, 510], [510, 510], [510, 510], [768, 768]],
        saturated=[0, 0, 0, 0, 0, 0, 0, 0], clear=1.0, min_margin=1.000),
    'xcd_v8': dict(depths=[3, 2, 5, 3, 7, 4, 6, 2, 8, 4, 10, 5, 8, 3, 10, 4],
        kept=[3, 2, 5, 3, 7, 4, 6, 2, 8, 4, 9, 5, 8, 3, 10, 4],
        last=[[1, 2], [0, 1], [3, 4], [1, 2], [5, 6], [2, 3], [4, 5], [0, 1], [6, 7], [1, 3], [8, 8], [2, 4], [7, 7], [0, 2], [9, 9], [1, 3]],
        saturated=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.091),
    'sat_v9': dict(depths=[34, 84, 85, 86, 276, 277, 278, 532, 533],
        kept=[34, 42, 42, 42, 42, 42, 42, 42, 42],
        last=[[12, 12], [62, 62], [63, 63], [64, 64], [254, 254], [255, 255], [256, 256], [510, 510], [511, 511]],
        saturated=[256, 256, 256, 256, 256, 256, 256, 256, 256], clear=1.0, min_margin=0.130),
    'fsat_v5': dict(depths=[276, 277, 278, 532, 533],
        kept=[276, 277, 278, 532, 533],
        last=[[254, 254], [255, 255], [256, 256], [510, 510], [511, 511]],
        saturated=[256, 256, 256, 256, 256], clear=1.0, min_margin=0.192),
    'sat_wave': dict(depths=[149, 277],
        kept=[149, 277],
        last=[[63, 63], [191, 191]],
        saturated=[256, 256], clear=1.0, min_margin=0.046),
    'fhard_v8': dict(depths=[256, 256, 256, 256, 256, 256, 256, 256],
        kept=[256, 256, 256, 256, 256, 256, 256, 256],
        last=[[255, 255], [255, 255], [255, 255], [255, 255], [255, 255], [255, 255], [255, 255], [255, 255]],
        saturated=[0, 0, 0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.272),
    'sat_partial_0': dict(depths=[19],
        kept=None,
        last=[[12, 13]],
        saturated=[256], clear=1.0, min_margin=0.074),
    'sat_partial_242': dict(depths=[261],
        kept=[19],
        last=[[254, 255]],
        saturated=[256], clear=1.0, min_margin=0.074),
    'eq256': dict(depths=[256, 256, 256, 256, 256, 256],
        kept=[256, 256, 256, 256, 256, 256],
        last=[[255, 255], [255, 255], [255, 255], [255, 255], [255, 255], [255, 255]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=2.052),
    'eq257_v2': dict(depths=[257, 257, 257, 257, 257, 257, 70, 70, 70, 70, 70, 70],
        kept=[257, 257, 257, 257, 257, 257, 70, 70, 70, 70, 70, 70],
        last=[[256, 256], [256, 256], [256, 256], [256, 256], [256, 256], [256, 256], [61, 61], [61, 61], [61, 61], [61, 61], [61, 61], [61, 61]],
        saturated=[0, 0, 0, 0, 0, 0, 256, 256, 80, 80, 80, 25], clear=1.0, min_margin=0.310),
    'uneq': dict(depths=[73, 8, 0, 5, 5, 0],
        kept=[73, 8, 0, 5, 5, 0],
        last=[[72, 72], [7, 7], [-1, -1], [4, 4], [4, 4], [-1, -1]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=2.051),
    'cell256': dict(depths=[260],
        kept=[260],
        last=[[259, 259]],
        saturated=[0], clear=1.0, min_margin=0.310),
    'cell_lens': dict(depths=[224, 197],
        kept=[224, 197],
        last=[[30, 223], [64, 196]],
        saturated=[0, 0], clear=1.0, min_margin=0.277),
    'hard_v9': dict(depths=[256, 256, 256, 256, 256, 256, 256, 256, 256],
        kept=[64, 65, 64, 65, 64, 65, 64, 65, 64],
        last=[[252, 252], [252, 252], [252, 252], [255, 255], [252, 252], [252, 252], [252, 252], [255, 255], [252, 252]],
        saturated=[0, 0, 0, 0, 0, 0, 0, 0, 0], clear=1.0, min_margin=1.000),
    'needle': dict(depths=[34, 34, 33, 33, 33, 33],
        kept=[34, 34, 33, 33, 33, 33],
        last=[[33, 33], [33, 33], [32, 32], [32, 32], [32, 32], [32, 32]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.049),
    'chunks': dict(depths=[265, 118, 116, 117, 117, 116],
        kept=[152, 2, 2, 2, 2, 2],
        last=[[264, 264], [117, 117], [115, 115], [116, 116], [116, 116], [115, 115]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.087),
    'gather': dict(depths=[88, 88, 4, 67, 67, 5],
        kept=[88, 67, 3, 66, 66, 4],
        last=[[87, 87], [87, 87], [3, 3], [66, 66], [66, 66], [4, 4]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.087),
    'sharp300': dict(depths=[163, 176, 75, 88, 70, 38],
        kept=[133, 127, 60, 67, 48, 29],
        last=[[154, 162], [170, 174], [72, 74], [82, 86], [66, 69], [37, 37]],
        saturated=[0, 0, 0, 0, 0, 0], clear=1.0, min_margin=0.091),
    'onehot16': dict(depths=[21],
        kept=None,
        last=[[20, 20]],
        saturated=[0], clear=1.0, min_margin=0.091),
    'duplicated': dict(depths=[38],
        kept=None,
        last=[[12, 13]],
        saturated=[256], clear=1.0, min_margin=0.074),
    'edge_1x1': dict(depths=[23],
        kept=None,
        last=[[12, 12]],
        saturated=[1], clear=1.0, min_margin=0.127),
    'edge_row33': dict(depths=[22, 22, 21],
        kept=None,
        last=[[13, 14], [13, 14], [11, 11]],
        saturated=[16, 16, 1], clear=1.0, min_margin=0.042),
    'edge_col17': dict(depths=[23, 21],
        kept=None,
        last=[[14, 15], [11, 11]],
        saturated=[16, 1], clear=1.0, min_margin=0.044),
    'edge_15': dict(depths=[23, 23],
        kept=[23, 23],
        last=[[13, 15], [13, 15]],
        saturated=[225, 225], clear=1.0, min_margin=0.043),
    'edge_17x31': dict(depths=[22, 20, 22, 21],
        kept=[22, 20, 22, 21],
        last=[[13, 14], [12, 12], [13, 14], [11, 13]],
        saturated=[256, 16, 240, 15], clear=1.0, min_margin=0.042),
    'edge_32x16': dict(depths=[22, 22],
        kept=[22, 22],
        last=[[13, 14], [12, 14]],
        saturated=[256, 256], clear=1.0, min_margin=0.041),
}


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_is_what_it_was_built_for(name, oracle_built):
    got, pin = measure(name), PINS[name]
    assert got["depths"] == pin["depths"]
    assert got["kept"] == pin["kept"]
    if pin["kept"] is not None:
        # independent of the rectangle rule restated in fused_kept_depths: nothing that passes the alpha test on some pixel
        # of a tile may be missing from its kept list, and nothing is kept that the reference list does not have
        need = bc.alpha_hit_counts(bc.get(name)).reshape(-1).tolist()
        assert all(n <= k <= d for n, k, d in zip(need, pin["kept"], pin["depths"])), (need, pin["kept"])
    assert got["last"] == pin["last"]
    assert got["saturated"] == pin["saturated"]
    # the cap: every pixel of every case counts (flat / sharp cases must reach exactly 1.0, needle cases >= 0.99)
    assert got["clear"] == pin["clear"] == 1.0
    assert got["min_margin"] >= pin["min_margin"] > 1e-2


def test_planted_depths_and_saturation_indices(oracle_built):
    """by construction, not by measurement"""
    assert PINS["depth_v9"]["depths"] == [0, 1, 3, 4, 5, 63, 64, 65, 0]
    assert PINS["depth_v8"]["depths"] == [255, 256, 257, 0, 511, 512, 513, 769]
    assert all(s == 0 for s in PINS["depth_v9"]["saturated"] + PINS["depth_v8"]["saturated"])
    # every pixel saturates at list index s: the last blended record is s - 1, with 20 live records behind index s
    assert PINS["sat_v9"]["last"] == [[s - 1, s - 1] for s in bc.SAT_AT]
    assert PINS["sat_v9"]["depths"] == [s + 21 for s in bc.SAT_AT]
    assert PINS["sat_v9"]["saturated"] == [256] * 9
    assert PINS["fsat_v5"]["last"] == [[s - 1, s - 1] for s in bc.FSAT_AT]
    assert PINS["fsat_v5"]["kept"] == PINS["fsat_v5"]["depths"] == [s + 21 for s in bc.FSAT_AT]
    # the sharp record at index 255 saturates some pixels of quadrant 0, the flat one at 256 all the others
    assert PINS["sat_partial_242"]["last"] == [[254, 255]] and PINS["sat_partial_242"]["depths"] == [261]
    assert PINS["sat_partial_0"]["last"] == [[12, 13]]
    assert PINS["eq256"]["depths"] == PINS["eq256"]["kept"] == [256] * 6
    assert PINS["eq257_v2"]["depths"][:6] == [257] * 6
    assert PINS["uneq"]["depths"] == [73, 8, 0, 5, 5, 0]                  # list starts 73, 81, 81, 86: mid-word
    # one wave finished (its 64 pixels saturate one by one at the pins, indices B - 64 .. B - 1), the others at index B
    assert PINS["sat_wave"]["last"] == [[B - 65, B - 65] for B in bc.SAT_WAVE_AT]
    assert PINS["sat_wave"]["kept"] == PINS["sat_wave"]["depths"] == [B + 21 for B in bc.SAT_WAVE_AT]
    for c, (B, q) in enumerate(zip(bc.SAT_WAVE_AT, (0, 3))):
        T = 1.0 - bc.reference("sat_wave")["f64"]["alpha"][c, :, :, 0]
        quad = np.zeros((16, 16), bool); quad[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] = True
        # the pinned quadrant stopped before its pin (T = 1.2e-4 kept), every other pixel before the record at B (same T)
        assert np.all((T > 1.0e-4) & (T < 1.4e-4))
        hits = bc.alpha_hit_counts(bc.get("sat_wave"), cell=8)[c].reshape(-1)
        assert hits[q] - hits[(q + 1) % 4] == 64                            # the 64 pins reach that quadrant alone
    # the fused path keeps whole batches around the single hard record
    assert PINS["fhard_v8"]["kept"] == PINS["fhard_v8"]["depths"] == [256] * 8
    fh = bc.get("fhard_v8")
    for c in range(8):
        hard = np.nonzero(fh.opacities[c * 256:(c + 1) * 256] > 0.998)[0].tolist()
        assert hard == [bc.HARD_POS[c % 4]]
    assert len(set(PINS["xcd_v8"]["depths"][0::2])) >= 6 and len(PINS["xcd_v8"]["depths"]) == 16
    # cell lists of the first batch of cell256, counted from the alpha test itself: wave 0's four cells hold (0, 1, 33, 256)
    cells = bc.alpha_hit_counts(bc.get("cell256"), cell=4, first=256)[0]
    assert (cells[0, 0], cells[0, 1], cells[1, 0], cells[1, 1]) == (0, 1, 33, 256) and cells.sum() == 290
    lens = bc.alpha_hit_counts(bc.get("cell_lens"), cell=4)
    assert lens[0].reshape(-1).tolist() == [31, 32, 63, 64, 33, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert lens[1].reshape(-1).tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 65, 1, 30, 34, 2, 3, 62, 0]
    # chunks: contributing records per wave (quadrant) and backward round of 64 list positions in tile 0
    ch = bc.get("chunks")
    per_round = []
    for r in range(4):
        sub = bc.Case("r", ch.records[64 * r:64 * r + 64].copy(), 1, 64, 16, 16)
        per_round.append(bc.alpha_hit_counts(sub, cell=8)[0].reshape(-1).tolist())
    assert per_round == [[1, 2, 3, 5], [1, 63, 0, 0], [0, 0, 64, 0], [4, 0, 0, 0]]
    assert PINS["cell256"]["depths"] == [260] and PINS["hard_v9"]["depths"] == [256] * 9
    assert PINS["duplicated"]["depths"] == [38] and PINS["duplicated"]["last"] == PINS["sat_partial_0"]["last"]
    case = bc.get("gather")
    tpg = case.lists()[0]
    cum = np.cumsum(tpg)
    assert case.Cn * case.N > 256 and (tpg == 0).sum() >= 2
    assert tpg[254] == 6 and cum[253] == 254 and cum[254] == 260        # slots 254 .. 259 cross a 256-slot window
    assert sorted(set(bc.get("chunks").lists()[0].tolist())) == [1, 2, 4, 6]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_oracle_agrees_with_the_float64_blend(name, oracle_built):
    """oracle/gs_oracle.c (float pixel arithmetic) against blend_cases.ref64 (float64, vectorised, written independently):
    image, last_ids, and every gradient -- the difference is the float32 evaluation's own error, from which the GPU test
    takes its bounds.  Largest where pixels saturate: gsplat's backward starts from T_final = 1 - alpha, and alpha =
    0.99988 carries half an ulp (3e-8) of absolute error into a T_final of 1.2e-4."""
    R = bc.reference(name)
    np.testing.assert_allclose(R["fwd"]["rgb"], R["f64"]["rgb"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(R["fwd"]["alpha"], R["f64"]["alpha"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(R["fwd"]["last"], R["f64"]["last"])
    for has_va in (True, False):
        for k, b in R["bwd"][has_va]["bounds"].items():
            assert b["scale"] > 0 and b["own"] <= 3e-3 * b["scale"], (name, has_va, k, b["own"] / b["scale"])
    for k, b in R["depth"]["bounds"].items():
        assert b["own"] <= 3e-3 * b["scale"], (name, "depth", k, b["own"] / b["scale"])


def test_an_empty_first_tile_passes_no_gradient(oracle_built):
    """gso_blend_bwd used to start at last_ids == 0 for the pixels of an empty tile in front of the first record and walked
    the first record of ANOTHER tile (gsplat does not: the tile has no batch).  depth_v9's view 0 is such a tile."""
    case = bc.get("depth_v9"); R = bc.reference("depth_v9")
    v_rgb = np.zeros_like(R["v_rgb"]); v_rgb[0] = 1.0                      # cotangent on the empty view only
    g = bc.oracle_bwd(case, R["fwd"], v_rgb, None)
    assert all(not g[k].any() for k in bc.GRAD_KEYS)
