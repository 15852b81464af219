"""Hand-written inputs that plant the edges of the fused front end's own tiling (no torch, no GPU): k_records_prepare /
k_project_sh_fwd (level-1 keys, rectangles), k_scan_chained, k_isect_gather / k_isect_wg_scan / k_isect_emit_d, the
segmented and device-count radix sorts, k_isect_offsets32.

Used by test_oracle_front.py (CPU pins of every planted property, and the paths reached, through st3r_front_plan) and
test_gpu_front.py (the kernels against oracle/gs_oracle.c: exact integers).  Two kinds of case:

  record cases  [Cn * N, 12] records in the pipeline's own layout (blend_cases.py), for ops.raster_train and the stage
                calls.  Every live record is of the FLAT kind of blend_cases (conic 1e-7, opacity 0.5): its alpha >= 1/255
                box spans ~9850 px, so tight_tile_rect keeps the whole reference rectangle and the fused list is the
                oracle's list, nothing left out (test_oracle_front.py asserts it per pair).  Mean and radius are chosen
                so that ref_tile_rect is a wanted rectangle: `tl` = tiles [0, w) x [0, h), `br` = the same size in the
                bottom right corner, `one` = a single tile, `none` = a visible record whose square misses the image (no
                tile; it keeps its place in the depth order).  The depth field is a float32 BIT PATTERN (BASE + rank in
                the order a case adds its records, unless given); radius 0 is a culled pair (level-1 sentinel: sorts last).
                A case lists a camera's records in DEPTH order and scatters them over the pair ids with a permutation, so
                that the emission's gather is a real one.
  scene cases   Gaussians for ops.train_fwd_bwd / ops.render / ops.rasterization under the identity camera of
                kat_scenes.cam_front (z = means[:, 2] exactly) or the same turned by pi about y (z = -means[:, 2]):
                isotropic, unit quaternions, opacity 0.9, sigma 8 px on the image (radius 25 < the alpha box's 26.5: tight
                == reference again), depths from bit patterns.  Culled Gaussians are all-zero rows (z = 0 < near).

A case keeps only its LIVE rows (`live_pid`, `live_rows` / `live`): the expected lists come from the oracle run on those
rows alone, mapped back to dense pair ids, and the GPU test builds the dense tensors on the device with torch.zeros plus
an indexed write -- the same code for 6 pairs and for the 16.8 M pairs of `wg_scan`.
"""
import math

import numpy as np

import blend_cases as bc

TILE = bc.TILE

# The tiling constants of the front end, restated once.  test_oracle_front.py asserts them against st3r_front_plan, which
# reports the values the library was compiled with: a retuned constant fails there instead of thinning the coverage.
SCAN_TILE = 4096              # gs_isect.hip: elements per workgroup of k_scan_chained
LOOKBACK = 256                # predecessors per trip of chain_lookback256
EP = 1024                     # pairs per emission workgroup
ECH = 4096                    # outputs per emission chunk
EMIT_SELF_BASE_MAX = 16384    # above this many emission workgroups k_isect_wg_scan runs
SORT_TILE_S32, SORT_TILE_L32 = 512 * 8, 1024 * 16      # radix_sort.hip: items per tile, 32-bit keys, small / large shape
SORT_TILE_S64, SORT_TILE_L64 = 512 * 4, 1024 * 8
RS_SMALL_BELOW = 100          # fewer large tiles than this: the small shape
OFFSET_KEYS = 4               # keys per thread of k_isect_offsets32


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


NEAR_BITS, FAR_BITS = f32_bits(0.01), f32_bits(1e10)
BASE = f32_bits(1.0)          # 0x3F800000


def passes_for(lo_bits, hi_bits):
    """(bias, sentinel, passes) that k_reg_reduce leaves in counts[8..10] for live depth codes lo .. hi: the keys are
    biased by the smallest one, the culled pairs get span + 1, and the segmented sort runs as many 8-bit passes as that
    sentinel needs (top < 2^8 / 2^16 / 2^24)."""
    if lo_bits is None:
        return (0, 1, 1)
    top = hi_bits - lo_bits + 1
    return (lo_bits - NEAR_BITS, top, 1 if top < 1 << 8 else 2 if top < 1 << 16 else 3 if top < 1 << 24 else 4)


# ---------------------------------------------------------------------------------------------------------------------
# record cases
NONE_XY, NONE_RADIUS = -1000.0, 4


class RecordCase:
    def __init__(self, name, W, H, Cn, N, live_pid, live_rows, fill=None):
        """live_pid ascending dense pair ids (camera * N + index), live_rows [L, 12] with radius > 0.  fill: None = every
        other row is a culled record (all zero), else the 12 floats of every other row (a `none` record)."""
        self.name, self.W, self.H, self.Cn, self.N = name, W, H, Cn, N
        self.tw, self.th = math.ceil(W / TILE), math.ceil(H / TILE)
        self.n_tiles = self.tw * self.th
        self.n_pairs = Cn * N
        order = np.argsort(live_pid, kind="stable")
        self.live_pid = np.asarray(live_pid, np.int64)[order]
        self.live_rows = np.ascontiguousarray(np.asarray(live_rows, np.float32)[order])
        assert self.live_pid.size == np.unique(self.live_pid).size and (self.radii() > 0).all()
        self.fill = None if fill is None else np.asarray(fill, np.float32)
        self._lists = None

    def radii(self):
        return np.ascontiguousarray(self.live_rows[:, 10]).view(np.int32)

    def dbits(self):
        return np.ascontiguousarray(self.live_rows[:, 9]).view(np.uint32)

    def cams(self):
        return (self.live_pid // self.N).astype(np.int32)

    def dense(self):
        """[Cn * N, 12] on the host (small cases only)"""
        assert self.n_pairs <= 1 << 20, "build this one on the device"
        rec = np.zeros((self.n_pairs, 12), np.float32)
        if self.fill is not None:
            rec[:] = self.fill
        rec[self.live_pid] = self.live_rows
        return rec

    def rects(self):
        """(reference, tight) rectangles of the live rows, [L, 4] = x0, x1, y0, y1 (blend_cases.tile_rects)"""
        r = self.live_rows
        return bc.tile_rects(r[:, 0:2], self.radii(), r[:, 2], r[:, 3:6], self.tw, self.th)

    def lists(self):
        """From the CPU oracle: tpg (tiles per live row), flat (sorted DENSE pair ids), off ([Cn * tiles + 1], the total
        closes the last tile), keys (sorted 32-bit (camera, tile) keys), n."""
        if self._lists is None:
            from oracle import gs_oracle as go
            r = self.live_rows
            tpg, ids, flat = go.isect_tiles(np.ascontiguousarray(r[:, 0:2]), self.radii(), np.ascontiguousarray(r[:, 9]),
                                            self.cams(), TILE, self.tw, self.th)
            ids_s, flat_s = go.sort_pairs(ids, flat)
            off = go.isect_offsets(ids_s, self.Cn, self.tw, self.th)
            tb = int(self.n_tiles).bit_length()
            hi = ids_s >> 32
            keys = (hi >> tb) * self.n_tiles + (hi & ((1 << tb) - 1))
            self._lists = dict(tpg=tpg, ids_unsorted=ids, flat_unsorted=self.live_pid[flat], ids=ids_s,
                               flat=self.live_pid[flat_s], off=np.append(off.reshape(-1), flat_s.size).astype(np.int32),
                               off3=off, keys=keys, n=int(flat_s.size))
        return self._lists

    def depth_order(self, cam):
        """indices into the live rows of camera `cam` in level-1 order: depth bits, then pair id"""
        sel = np.nonzero(self.cams() == cam)[0]
        return sel[np.lexsort((self.live_pid[sel], self.dbits()[sel]))]

    def workgroups(self, cam):
        """Per emission workgroup (EP consecutive pairs of the camera's depth order; the pairs that are not live rows come
        behind them when they are culled -- fill None -- and are asserted to be nowhere else by the cases that use a fill):
        list of the tile counts of its pairs, live rows only, in order."""
        tpg = self.lists()["tpg"]
        order = self.depth_order(cam)
        return [tpg[order[k:k + EP]].tolist() for k in range(0, max(len(order), 1), EP)]


def flat_row(x, y, radius, dbits, rng):
    row = np.zeros(12, np.float32)
    row[0:2] = (x, y); row[2] = 0.5; row[3:6] = bc.FLAT_CONIC; row[6:9] = rng.uniform(0.1, 0.9, 3)
    row[9:11] = np.array([dbits, radius], np.uint32).view(np.float32)
    return row


class Records:
    """Builder: per camera a list of records in DEPTH order."""

    def __init__(self, name, W, H, Cn, N=None, seed=0, shuffle=True):
        self.name, self.W, self.H, self.Cn, self.N = name, W, H, Cn, N
        self.tw, self.th = math.ceil(W / TILE), math.ceil(H / TILE)
        self.order = [[] for _ in range(Cn)]
        self.rng = np.random.default_rng(4321 + seed)
        self.shuffle = shuffle

    def _add(self, cam, x, y, radius, n, dbits):
        for _ in range(n):
            self.order[cam].append((float(x), float(y), int(radius), dbits))
        return self

    def tl(self, cam, w, h, n=1, dbits=None):
        """tiles [0, w) x [0, h): the square ends half a tile inside column w - 1 / row h - 1 and starts left of / above 0"""
        assert 1 <= w <= self.tw and 1 <= h <= self.th
        r = 16 * max(w, h) + 200
        return self._add(cam, 16 * w - 8 - r, 16 * h - 8 - r, r, n, dbits)

    def br(self, cam, w, h, n=1, dbits=None):
        """tiles [tw - w, tw) x [th - h, th)"""
        assert 1 <= w <= self.tw and 1 <= h <= self.th
        r = 16 * max(w, h) + 200
        return self._add(cam, 16 * (self.tw - w) + 8 + r, 16 * (self.th - h) + 8 + r, r, n, dbits)

    def one(self, cam, tx, ty, n=1, dbits=None):
        assert 0 <= tx < self.tw and 0 <= ty < self.th
        return self._add(cam, 16 * tx + 8, 16 * ty + 8, 4, n, dbits)

    def key(self, k, n=1, dbits=None):
        """one tile, given as its (camera, tile) key"""
        t = k % (self.tw * self.th)
        return self.one(k // (self.tw * self.th), t % self.tw, t // self.tw, n, dbits)

    def none(self, cam, n=1, dbits=None):
        return self._add(cam, NONE_XY, NONE_XY, NONE_RADIUS, n, dbits)

    def area(self, cam, a):
        """pairs whose tile counts add up to `a`, the largest rectangles first"""
        full = self.tw * self.th
        while a >= full:
            self.tl(cam, self.tw, self.th); a -= full
        if a >= self.tw:
            self.tl(cam, self.tw, a // self.tw); a %= self.tw
        if a:
            self.tl(cam, a, 1)
        return self

    def pad(self, cam):
        """`none` records up to the end of the emission workgroup"""
        return self.none(cam, (-len(self.order[cam])) % EP)

    def block(self, cam, total):
        """one whole emission workgroup of `total` outputs"""
        assert len(self.order[cam]) % EP == 0
        self.area(cam, total)
        assert len(self.order[cam]) % EP != 0 or total == 0
        return self.none(cam, EP) if total == 0 else self.pad(cam)

    def build(self):
        Cn = self.Cn
        N = self.N if self.N is not None else max(1, max(len(o) for o in self.order))
        pid, rows = [], []
        for c in range(Cn):
            L = len(self.order[c])
            assert L <= N, (self.name, c, L, N)
            slots = self.rng.permutation(N)[:L] if self.shuffle else np.arange(L)
            for rank, (x, y, radius, dbits) in enumerate(self.order[c]):
                pid.append(c * N + int(slots[rank]))
                rows.append(flat_row(x, y, radius, BASE + rank if dbits is None else dbits, self.rng))
        rows = np.array(rows, np.float32).reshape(-1, 12)
        return RecordCase(self.name, self.W, self.H, Cn, N, np.array(pid, np.int64), rows)


def _random_records(name, W, H, Cn, N, seed, p_live=0.35, p_none=0.3):
    """every camera another random mix of rectangles, tile-less records and culled pairs (the pairs left over)"""
    b = Records(name, W, H, Cn, N, seed)
    rng = np.random.default_rng(77 + seed)
    for c in range(Cn):
        n_vis = int(N * (0.5 + 0.5 * rng.random())) if c % 4 != 3 else (N if c % 8 == 3 else 0)
        for _ in range(n_vis):
            u = rng.random()
            if u < p_live:
                w, h = int(rng.integers(1, b.tw + 1)), int(rng.integers(1, b.th + 1))
                (b.tl if rng.random() < 0.5 else b.br)(c, w, h)
            elif u < p_live + p_none:
                b.none(c)
            else:
                b.one(c, int(rng.integers(0, b.tw)), int(rng.integers(0, b.th)))
    return b.build()


# ---- the scan with rectangles: N * C on both sides of one scan tile ----
def scan_rects(n):
    return _random_records("scan_rects_%d" % n, 48, 32, 1, n, n)


# ---- emission ----
EMIT_TOTALS = [0, 1, ECH - 1, ECH, ECH + 1, 3 * ECH]
LIVE_AT = [0, 255, 256, 1023]


def emit_totals():
    """96 x 64 (6 x 4 tiles), three cameras, N = 8 * EP + 1.
    camera 0: workgroups of 0, 1, 4095, 4096, 4097 and 3 x 4096 outputs; one of 4095 outputs followed by a 6-tile pair whose
              first output is output 4095 (the last entry of chunk 0) and three 1-tile pairs; one of 4096 outputs followed by
              a 6-tile pair whose first output is output 4096 (the first entry of chunk 1); a last workgroup of ONE pair.
    camera 1: the same workgroups in reverse order; the last workgroup (1 pair) is a culled pair.
    camera 2: live pairs only at positions 0, 255, 256 and 1023 of the first workgroup (24 tiles each: the last pairs of
              every 256-pair scan but one are empty), an all-empty workgroup, one whose last 1000 pairs are all empty,
              then 1023 visible pairs in the last whole workgroup; the rest culled."""
    b = Records("emit_totals", 96, 64, 3, 8 * EP + 1, 1)
    blocks = [lambda c, t=t: b.block(c, t) for t in EMIT_TOTALS]
    blocks.append(lambda c: (b.area(c, ECH - 1), b.tl(c, 3, 2), b.one(c, 1, 1, 3), b.pad(c)))
    blocks.append(lambda c: (b.area(c, ECH), b.tl(c, 3, 2), b.one(c, 5, 3, 2), b.pad(c)))
    for f in blocks:
        f(0)
    b.one(0, 2, 2)                                  # workgroup 8 of camera 0: one pair
    for f in reversed(blocks):
        f(1)
    for p in range(EP):
        b.tl(2, 6, 4) if p in LIVE_AT else b.none(2)
    b.none(2, EP)
    b.tl(2, 6, 4, 24).none(2, EP - 24)
    b.one(2, 0, 0, 1023)
    return b.build()


def emit_big():
    """4080 x 768 (255 x 48 tiles: the 32-bit rectangle form's widest grid), one camera, one workgroup:
    a 1-tile pair (output 0); a pair of 241 x 17 = 4097 tiles from output 1 -- chunk 1 starts with two outputs of it and no
    mark --; three 1-tile pairs; a pair of 255 x 48 = 12 240 tiles (chunk 2 holds no mark at all) followed by five
    1-tile pairs; a pair of 255 x 33 = 8415 tiles (chunks 4 and 5: no mark); 1-tile pairs; culled pairs behind."""
    b = Records("emit_big", 4080, 768, 1, 40, 2)
    b.one(0, 0, 0).tl(0, 241, 17).one(0, 254, 47, 3).tl(0, 255, 48).one(0, 7, 7, 5).br(0, 255, 33).one(0, 100, 20, 4)
    return b.build()


WIDTHS = [1, 2, 3, 5, 7, 15, 17]


def emit_widths():
    """272 x 64 (17 x 4 tiles): every width of WIDTHS with heights 1 .. 4, from the top left and from the bottom right corner:
    every index kk in [0, w h) of the row / column decode (kk / w through v_rcp_f32 and its two corrections)"""
    b = Records("emit_widths", 272, 64, 2, None, 3)
    for w in WIDTHS:
        for h in (1, 2, 3, 4):
            b.tl(0, w, h).br(0, w, h).br(1, w, h).tl(1, w, h)
    return b.build()


def emit_strip(name, W, H, seed):
    """strip images: 4080 x 48 (255 x 3), 48 x 4080 (3 x 255), 4112 x 48 (257 x 3: 64-bit rectangles by the grid's width)"""
    b = Records(name, W, H, 1, None, seed)
    for w, h in ((b.tw, 1), (b.tw, b.th), (b.tw - 1, b.th), (1, b.th), (min(b.tw, 3), min(b.th, 3)), (b.tw, max(1, b.th - 1))):
        b.tl(0, w, h).br(0, w, h)
    return b.build()


def emit_cams(Cn, N, seed):
    """48 x 32; 8 / 16 views with one and three workgroups per camera (the workgroup-to-camera map is interleaved), 3 / 9
    views (the plain map); N = 1025 and 2047: a last workgroup of 1 and of 1023 pairs; cameras 3, 11: everything visible,
    cameras 7, 15: everything culled"""
    return _random_records("emit_cams_%d_%d" % (Cn, N), 48, 32, Cn, N, seed, p_live=0.1, p_none=0.6)


# ---- tile sort and offsets ----
def offs_keys(total):
    """C * tiles = 1, 2, 255, 256, 257 (end_bit 0 -> 1, 1, 8, 8, 9): records in the first, a middle and the last key"""
    W, H, Cn = {1: (16, 16, 1), 2: (32, 16, 1), 255: (272, 80, 3), 256: (128, 128, 4), 257: (4112, 16, 1)}[total]
    b = Records("offs_keys_%d" % total, W, H, Cn, None, total)
    assert b.tw * b.th * Cn == total
    for k, n in ((0, 2), (total // 2, 3), (total - 1, 1 + total % 4)):
        b.key(k, n)
    return b.build()


def offs_pattern(which, extra):
    """320 x 256 (20 x 16 = 320 tiles), one camera; `extra` more records in the last occupied tile move n % 4.
    first: only tile 0; last: only tile 319; second: every second tile; gap: tiles 7 and 308 with a run of 300 empty keys
    between them (the thread that holds the record of tile 308 fills 301 entries, across its neighbours' ranges);
    runs: empty keys in front (9), in the middle (100) and behind (50)"""
    b = Records("offs_%s_%d" % (which, extra), 320, 256, 1, None, 10 * extra + len(which))
    keys = dict(first=[0], last=[319], second=list(range(1, 320, 2)), gap=[7, 308],
                runs=list(range(9, 120)) + list(range(220, 270)))[which]
    for k in keys:
        b.key(k, 1 if which == "second" else 3)
    b.key(keys[-1], extra)
    return b.build()


# ---- recipes for the device-built cases ----
def keys_65552():
    """16 views of 3856 x 272 (241 x 17 = 4097 tiles): 65 552 (camera, tile) keys, end_bit 17 -- three passes of the tile
    sort.  Three records: the first key, a middle one and the last."""
    b = Records("keys_65552", 3856, 272, 16, 1, 5)
    b.one(0, 0, 0).one(8, 120, 8).one(15, 240, 16)
    return b.build()


def wg_scan():
    """N = 2 097 153 + 1024, 8 views: ceil(N / EP) = 2050 workgroups per camera, 16 400 in all > EMIT_SELF_BASE_MAX, so the
    emission takes its base from k_isect_wg_scan.  Every row that is not planted is a `none` record with the depth bits
    BASE: all tied, so the level-1 order is the pair-id order and a planted record with the same bits sits at its own
    index.  Planted: the first workgroup of camera 0 (positions 0, 1, 1023), workgroup 16 384 of the launch = workgroup 2048
    of camera 0 (first and last pair), the middle of camera 3, camera 5's first workgroup, and the last, ragged workgroup of
    camera 7 (one pair)."""
    N, Cn, W, H = 2097153 + 1024, 8, 48, 32
    rng = np.random.default_rng(6)
    fill = flat_row(NONE_XY, NONE_XY, NONE_RADIUS, BASE, rng)
    plant = [(0, 0, (3, 2)), (0, 1, (1, 1)), (0, 1023, (2, 2)), (0, 2048 * EP, (3, 1)), (0, 2048 * EP + 1023, (1, 2)),
             (3, 1000 * EP + 500, (3, 2)), (3, 1000 * EP + 501, (2, 1)), (5, 17, (1, 1)), (7, 5, (2, 2)), (7, N - 1, (3, 2))]
    pid, rows = [], []
    for cam, idx, (w, h) in plant:
        r = 16 * max(w, h) + 200
        pid.append(cam * N + idx)
        rows.append(flat_row(16 * w - 8 - r, 16 * h - 8 - r, r, BASE, rng))
    return RecordCase("wg_scan", W, H, Cn, N, np.array(pid, np.int64), np.array(rows, np.float32), fill=fill)


RECORD_CASES = {
    "scan_rects_4095": lambda: scan_rects(4095), "scan_rects_4096": lambda: scan_rects(4096),
    "scan_rects_4097": lambda: scan_rects(4097),
    "emit_totals": emit_totals, "emit_big": emit_big, "emit_widths": emit_widths,
    "emit_strip_255x3": lambda: emit_strip("emit_strip_255x3", 4080, 48, 11),
    "emit_strip_3x255": lambda: emit_strip("emit_strip_3x255", 48, 4080, 12),
    "emit_strip_257x3": lambda: emit_strip("emit_strip_257x3", 4112, 48, 13),
    "emit_cams_8_1000": lambda: emit_cams(8, 1000, 21), "emit_cams_8_2049": lambda: emit_cams(8, 2049, 22),
    "emit_cams_16_1000": lambda: emit_cams(16, 1000, 23), "emit_cams_16_2049": lambda: emit_cams(16, 2049, 24),
    "emit_cams_3_1025": lambda: emit_cams(3, 1025, 25), "emit_cams_9_2047": lambda: emit_cams(9, 2047, 26),
    "offs_keys_1": lambda: offs_keys(1), "offs_keys_2": lambda: offs_keys(2), "offs_keys_255": lambda: offs_keys(255),
    "offs_keys_256": lambda: offs_keys(256), "offs_keys_257": lambda: offs_keys(257),
    "offs_first_0": lambda: offs_pattern("first", 0), "offs_last_1": lambda: offs_pattern("last", 1),
    "offs_second_0": lambda: offs_pattern("second", 0), "offs_second_1": lambda: offs_pattern("second", 1),
    "offs_second_2": lambda: offs_pattern("second", 2), "offs_second_3": lambda: offs_pattern("second", 3),
    "offs_gap_2": lambda: offs_pattern("gap", 2), "offs_runs_3": lambda: offs_pattern("runs", 3),
    "keys_65552": keys_65552, "wg_scan": wg_scan,
}
# (the three large cases: keys_65552 and wg_scan here, and the scene `large`)


# ---------------------------------------------------------------------------------------------------------------------
# scene cases
F = 100.0
SIGMA_PX = 8.0


class SceneCase:
    def __init__(self, name, W, H, N, live_idx, zbits, sign, px, py, flip, seed):
        """live_idx ascending Gaussian indices; zbits the float32 bit patterns of their depths; sign +1: in front of the
        identity cameras, -1: in front of the turned ones (flip[c] True).  (px, py): where the Gaussian lands on a camera
        whose principal point is the image centre."""
        self.name, self.W, self.H, self.N = name, W, H, N
        self.C = len(flip)
        self.tw, self.th = math.ceil(W / TILE), math.ceil(H / TILE)
        self.n_tiles = self.tw * self.th
        self.n_pairs = self.C * N
        self.live_idx = np.asarray(live_idx, np.int64)
        assert np.all(np.diff(self.live_idx) > 0) if self.live_idx.size > 1 else True
        self.zbits = np.asarray(zbits, np.uint32)
        self.sign = np.asarray(sign, np.float64)
        z = self.zbits.view(np.float32).astype(np.float64)
        L = self.live_idx.size
        means = np.zeros((L, 3), np.float32)
        means[:, 0] = (self.sign * (np.asarray(px, np.float64) - W / 2) * z / F).astype(np.float32)
        means[:, 1] = ((np.asarray(py, np.float64) - H / 2) * z / F).astype(np.float32)
        means[:, 2] = (self.sign * z).astype(np.float32)
        assert np.array_equal(np.abs(means[:, 2]).view(np.uint32), self.zbits)
        rng = np.random.default_rng(999 + seed)
        sh = np.zeros((L, 24, 3), np.float32)
        sh[:, 0, :] = (rng.uniform(0.1, 0.9, (L, 3)) - 0.5) / 0.2820947917738781
        self.live = dict(means=means, quats=np.tile(np.array([1, 0, 0, 0], np.float32), (L, 1)),
                         scales=np.repeat((SIGMA_PX * z / F).astype(np.float32)[:, None], 3, 1),
                         opacities=np.full(L, 0.9, np.float32), shN=sh)
        self.flip = list(flip)
        self.viewmats = np.tile(np.eye(4, dtype=np.float32), (self.C, 1, 1))
        self.Ks = np.zeros((self.C, 3, 3), np.float32)
        for c in range(self.C):
            if flip[c]:
                self.viewmats[c, 0, 0] = -1.0; self.viewmats[c, 2, 2] = -1.0       # rotation by pi about y
            self.Ks[c] = [[F, 0, W / 2 + 3 * (c % 8)], [0, F, H / 2 - 2 * (c % 8)], [0, 0, 1]]
        self._ref = None

    def reference(self):
        """The oracle on the live Gaussians: meta of gs_oracle.rasterization plus, in DENSE pair ids, pid (of every packed
        pair), flat (sorted list), off ([C * tiles + 1]), and the level-1 key range (bias, sentinel, passes)."""
        if self._ref is None:
            from oracle import gs_oracle as go
            g = self.live
            if self.live_idx.size:
                rgb, alpha, meta = go.rasterization(g["means"], g["quats"], g["scales"], g["opacities"], g["shN"],
                                                    self.viewmats, self.Ks, self.W, self.H)
                pid = meta["camera_ids"].astype(np.int64) * self.N + self.live_idx[meta["gaussian_ids"]]
                flat = pid[meta["flatten_ids"]]
                off = np.append(meta["isect_offsets"].reshape(-1), flat.size).astype(np.int32)
                d = meta["depths"].view(np.uint32)
                kr = passes_for(int(d.min()), int(d.max())) if d.size else passes_for(None, None)
            else:
                rgb = np.zeros((self.C, self.H, self.W, 3), np.float32); alpha = np.zeros((self.C, self.H, self.W, 1), np.float32)
                meta = dict(tiles_per_gauss=np.zeros(0, np.int32), depths=np.zeros(0, np.float32),
                            means2d=np.zeros((0, 2), np.float32), radii=np.zeros(0, np.int32), conics=np.zeros((0, 3), np.float32),
                            opacities=np.zeros(0, np.float32), camera_ids=np.zeros(0, np.int32))
                pid = np.zeros(0, np.int64); flat = np.zeros(0, np.int64)
                off = np.zeros(self.C * self.n_tiles + 1, np.int32); kr = passes_for(None, None)
            self._ref = dict(meta=meta, rgb=rgb, alpha=alpha, pid=pid, flat=flat, off=off, krange=kr, n=int(flat.size))
        return self._ref


SPANS = [0, 254, 255, 256, 65534, 65535, 65536, (1 << 24) - 2, (1 << 24) - 1, 1 << 24, "near_far"]
SPAN_N = [4095, 4096, 4097, 8193]
SPAN_C = [1, 2, 7, 8]


def _span_bits(span, L, rng):
    """L depth codes whose smallest and largest are exactly `span` apart (both ends present, the rest random between)"""
    if span == "near_far":
        lo, hi = NEAR_BITS, FAR_BITS
    else:
        lo, hi = BASE, BASE + span
    z = rng.integers(lo, hi + 1, L, dtype=np.int64)
    z[int(rng.integers(0, L))] = lo
    free = np.nonzero(z != lo)[0] if L > 1 else np.zeros(0, int)
    z[free[0] if free.size else L - 1] = hi
    if L > 1 and span != 0:
        assert z.min() == lo and z.max() == hi
    return z.astype(np.uint32)


def _scene(name, N, flip, zbits_of, seed, culled_every=0, W=48, H=32):
    rng = np.random.default_rng(2024 + seed)
    idx = np.arange(N)
    if culled_every:
        idx = idx[idx % culled_every != 1]          # culled Gaussians interleaved: every culled_every-th index
    zb = zbits_of(idx.size, rng)
    px = rng.uniform(4, W - 4, idx.size); py = rng.uniform(4, H - 4, idx.size)
    return SceneCase(name, W, H, N, idx, zb, np.ones(idx.size), px, py, flip, seed)


def span_views(i, j, culled):
    """the view count rotates over the product: every span meets 1, 2, 7 and 8 views"""
    return SPAN_C[(i + j + int(culled)) % 4]


def span_name(span, N, culled):
    return "span_%s_n%d%s" % (span, N, "_culled" if culled else "")


def span_scene(i, j, culled):
    """span SPANS[i] x N = SPAN_N[j] x (every Gaussian live | every third one culled): the whole product, so that every pass
    count meets 1, 1, 2 and 3 sort tiles per segment with and without the culled pairs' sentinel among the keys"""
    span, N = SPANS[i], SPAN_N[j]
    return _scene(span_name(span, N, culled), N, [False] * span_views(i, j, culled), lambda L, rng: _span_bits(span, L, rng),
                  100 * i + 10 * j + int(culled), culled_every=3 if culled else 0)


TIE_GROUPS = [2, 3, 64, 65, 4097]


def ties_scene():
    """two identical cameras (the same depth bits in different cameras), N = 8193: groups of 2, 3, 64, 65 and 4097 Gaussians
    with identical depth bits, scattered over the indices (the 4097 over all three small sort tiles), everything else
    distinct; the expected order inside a group is the pair-id order"""
    def zbits(L, rng):
        z = BASE + 16 * (1 + rng.permutation(L)).astype(np.int64)
        who = rng.permutation(L)
        at = int(np.nonzero(who == L - 1)[0][0])
        big = sum(TIE_GROUPS[:-1])                   # the largest group is who[big : big + 4097]
        who[[at, big]] = who[[big, at]]              # the last index (a sort tile of its own when L = 8193) joins it
        k = 0
        for gi, sz in enumerate(TIE_GROUPS):
            z[who[k:k + sz]] = BASE + 16 * (L * (gi + 1) // 7) + 5      # between the distinct codes (those are multiples of 16)
            k += sz
        return z.astype(np.uint32)
    return _scene("ties", 8193, [False, False], zbits, 50)


def large_scene():
    """C = 8, N = 204 803, 32 x 16: 1 638 424 pairs = 400 scan tiles (two look-back trips) and 101 large sort tiles (the
    segmented sort's large shape: 13 tiles per segment, the last one ragged).  3000 planted Gaussians in the first, the
    middle and the last EP block of the indices, half of them in front of the identity cameras 0, 2, 5, 7, half in front of
    the turned cameras 1, 3, 4, 6; everything else is culled."""
    N, W, H = 204803, 32, 16
    rng = np.random.default_rng(88)
    idx = np.sort(np.concatenate([rng.choice(EP, 1000, replace=False), 100 * EP + rng.choice(EP, 1000, replace=False),
                                  N - EP + rng.choice(EP, 1000, replace=False)]))
    zb = (BASE + rng.integers(0, 1 << 20, idx.size)).astype(np.uint32)
    sign = np.where(rng.random(idx.size) < 0.5, 1.0, -1.0)
    px = rng.uniform(4, W - 4, idx.size); py = rng.uniform(4, H - 4, idx.size)
    return SceneCase("large", W, H, N, idx, zb, sign, px, py, [False, True, False, True, True, False, True, False], 88)


SCENE_CASES = {span_name(s, n, k): (lambda i=i, j=j, k=k: span_scene(i, j, k))
               for i, s in enumerate(SPANS) for j, n in enumerate(SPAN_N) for k in (False, True)}
for _j, _n in enumerate(SPAN_N):
    # nothing visible at all (every Gaussian is an all-zero row), two views
    SCENE_CASES["nothing_n%d" % _n] = lambda n=_n: SceneCase("nothing_n%d" % n, 48, 32, n, [], [], [], [], [], [False, False], 60)
    # camera 1 is turned away: every pair of it is culled while cameras 0 and 2 see everything
    for _k in (False, True):
        SCENE_CASES["blind_camera_n%d%s" % (_n, "_culled" if _k else "")] = (
            lambda n=_n, j=_j, k=_k: _scene("blind_camera_n%d%s" % (n, "_culled" if k else ""), n, [False, True, False],
                                            lambda L, rng: _span_bits(256, L, rng), 610 + 2 * j + int(k), culled_every=3 if k else 0))
SCENE_CASES.update({
    "views_9": lambda: _scene("views_9", 4097, [False] * 9, lambda L, rng: _span_bits(65536, L, rng), 62, culled_every=3),
    "views_16": lambda: _scene("views_16", 1000, [False] * 16, lambda L, rng: _span_bits(255, L, rng), 63),
    "ties": ties_scene,
    "large": large_scene,
})

_cache = {}


def get(name):
    """built once; of the scenes only the last few are kept (there are more than a hundred of them)"""
    if name not in _cache:
        scenes = [k for k in _cache if k in SCENE_CASES]
        if name in SCENE_CASES and len(scenes) >= 6:
            del _cache[scenes[0]]
        _cache[name] = (RECORD_CASES.get(name) or SCENE_CASES[name])()
    return _cache[name]


# ---- stand-alone scan ----
SCAN_SIZES = [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, (LOOKBACK - 1) * SCAN_TILE + 1, LOOKBACK * SCAN_TILE,
              LOOKBACK * SCAN_TILE + 1, (LOOKBACK + 1) * SCAN_TILE + 5, (2 * LOOKBACK + 1) * SCAN_TILE + 7]


def scan_counts(n, seed=0):
    """counts below 2^20 -- and small enough for a grand total below 2^31 -- with zeros among them (a third), and a run of
    zeros longer than a scan tile when n allows"""
    rng = np.random.default_rng(300 + seed + n % 1000)
    a = rng.integers(0, min(1 << 20, (2 ** 31 - 1) // n + 1), n).astype(np.int32)
    a[rng.random(n) < 0.33] = 0
    if n > 3 * SCAN_TILE:
        a[SCAN_TILE + 5:2 * SCAN_TILE + 9] = 0      # one whole tile of zeros and a bit
    return a


def scan_big_total(total):
    """2049 counts, each below 2^20, that add up to exactly `total` (2^31 - 1 or 2^31), then zeros to 2 * SCAN_TILE + 3"""
    n = 2049
    base = total // n
    a = np.full(n, base, np.int64)
    a[:total - base * n] += 1
    assert int(a.sum()) == total and a.max() < (1 << 20)
    out = np.zeros(2 * SCAN_TILE + 3, np.int32)
    out[np.random.default_rng(1).permutation(out.size)[:n]] = a
    return out


# ---- the host-side plan of a fused call (st3r_front_plan: host arithmetic, no GPU) ----
PLAN_FIELDS = ("rect32", "rectbase", "key32", "segments", "scan_tiles", "bpc", "emit_grid", "self_base", "l1_small", "l1_tile",
               "l1_tiles", "tiles_per_seg", "l1_passes", "end_bit", "ts_small", "ts_tile", "ts_tiles", "ts_passes")
PLAN_CONSTANTS = {20: "SCAN_TILE", 21: "EP", 22: "ECH", 23: "EMIT_SELF_BASE_MAX", 24: "OFFSET_KEYS", 25: "RS_SMALL_BELOW",
                  26: "SORT_TILE_S32", 27: "SORT_TILE_L32", 28: "SORT_TILE_S64", 29: "SORT_TILE_L64"}


def plan(N, C, W, H, flags=0, entry="train", n_records=0):
    """entry: 'train' (train_fwd_bwd / train_step), 'records' (raster_train) or 'render'"""
    import ctypes
    from starst3r_amd import _lib
    out = (ctypes.c_int64 * 32)()
    _lib.check(_lib.lib().st3r_front_plan(N, C, W, H, flags, int(entry == "train"), int(entry == "records"), n_records, out, 32))
    d = {k: int(out[i]) for i, k in enumerate(PLAN_FIELDS)}
    d.update({name: int(out[i]) for i, name in PLAN_CONSTANTS.items()})
    return d
