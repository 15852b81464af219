"""Hand-written splat records that plant the edges of the blend kernels' own tiling (no torch, no GPU).

Used by test_oracle_blend.py (CPU pins: per-tile list depths, saturation indices, clear fraction) and test_gpu_blend.py
(gs_blend.hip, gs_blend_cells.hip, gs_blend_depth.hip against oracle/gs_oracle.c).  A case is a set of records
[Cn * N, 12] in the pipeline's own layout

    x y opacity conic.a | conic.b conic.c r g | b depth radius-as-int-bits 0

The (record, tile) lists are never written by hand: they come from the oracle's isect_tiles / sort_pairs / isect_offsets
(CPU) or from ops.isect / ops.sort_pairs / ops.offsets (GPU, pinned bit-exact against the former), so `cum`, rectangles and
slots are consistent.  The depth field orders the records of a view (here: the order in which a case adds them; a tie
falls back to the pair id).  Records with radius 0 pad the views of a case to the same N and own no slot.

Two kinds of record keep every skip / stop decision far from its threshold (oracle margin, gso_blend_fwd):

  flat    mean well outside the image, conic (1e-7, 0, 1e-7), a radius that covers the tiles wanted: alpha is the opacity on
          every pixel to 4e-3, sigma ~ 2e-3 > 0.  Opacity 0.5 halves T: from T = 1 the 14th such record saturates a pixel
          (T 1.2e-4 -> 6.1e-5).  Opacity 0 is in the stand-alone lists and fails the alpha test; 0.012 contributes a little.
  sharp   conic (4, 0, 4), mean at a pixel centre + (-0.25, +0.25), radius 3: the pixel offsets are {-0.75, 0.25, 1.25} x
          {-1.25, -0.25, 0.75}, every alpha >= 8 % away from 1/255 for the opacities used here (0.9, 0.3, 0.02).  With
          opacity 0.02 the footprint is the three pixels (px, py), (px - 1, py), (px, py + 1) (alpha 0.0156, 0.0057, 0.0057;
          (px - 1, py + 1) gets 0.0021 < 1/255), with 0.9 / 0.3 three by three without the corner at distance (1.25, 1.25).
  pin     conic (20, 0, 20), opacity 0.9, same mean offset: alpha 0.258 on its own pixel, 0.0017 (0.44 / 255) on the nearest
          others -- one pixel and no more.

Tile = 16 x 16 pixels; a wave of the kernels owns an 8 x 8 quadrant, a 16-lane row of the cell forward a 4 x 4 cell; the
forward stages batches of 256 records, the backward rounds of 64 in chunks of 4.
"""
import math

import numpy as np

TILE = 16
FLAT_CONIC = (1e-7, 0.0, 1e-7)
SHARP_CONIC = (4.0, 0.0, 4.0)
PIN_CONIC = (20.0, 0.0, 20.0)
FILL = 0.012            # a contributing filler: 255 of them leave T = 0.046


class Builder:
    def __init__(self, name, W, H, Cn, seed=0, tie_depths=False):
        self.name, self.W, self.H, self.Cn = name, W, H, Cn
        self.recs = [[] for _ in range(Cn)]
        self.rng = np.random.default_rng(1234 + seed)
        self.tie = tie_depths

    def add(self, cam, x, y, op, conic, radius, n=1):
        for _ in range(n):
            col = self.rng.uniform(0.1, 0.9, 3)
            self.recs[cam].append((x, y, op, conic[0], conic[1], conic[2], col[0], col[1], col[2], int(radius)))
        return self

    def flat(self, cam, op, n=1):
        """covers every tile of images up to 48 x 32"""
        return self.add(cam, -150.0, -90.0, op, FLAT_CONIC, 400, n)

    def cflat(self, cam, op, tx1, ty1, n=1):
        """flat record whose rectangle is the tiles [0, tx1) x [0, ty1)"""
        r = 150 + 16 * tx1 - 8
        return self.add(cam, -150.0, float(-r + 16 * ty1 - 8), op, FLAT_CONIC, r, n)

    def sharp(self, cam, px, py, op=0.9, n=1, radius=3):
        return self.add(cam, px + 0.25, py + 0.75, op, SHARP_CONIC, radius, n)

    def pin(self, cam, px, py):
        return self.add(cam, px + 0.25, py + 0.75, 0.9, PIN_CONIC, 3)

    def fill(self, cam, n, every=1, other=0.0):
        """n flat fillers: opacity FILL at every `every`-th position, `other` (0: present but skipped) elsewhere"""
        for i in range(n):
            self.flat(cam, FILL if i % every == 0 else other)
        return self

    def build(self):
        Cn, N = self.Cn, max(1, max(len(r) for r in self.recs))
        rec = np.zeros((Cn * N, 12), np.float32)
        rad = np.zeros(Cn * N, np.int32)
        for c in range(Cn):
            for i, r in enumerate(self.recs[c]):
                k = c * N + i
                rec[k, 0:9] = r[0:9]
                rec[k, 9] = 1.0 if self.tie else 1.0 + 0.001 * i
                rad[k] = r[9]
            for i in range(len(self.recs[c]), N):       # padding: invisible, but a well-formed record
                rec[c * N + i, 0:10] = (-150.0, -90.0, 0.5, 1e-7, 0.0, 1e-7, 0.5, 0.5, 0.5, 2.0)
        rec[:, 10] = rad.view(np.float32)
        return Case(self.name, rec, Cn, N, self.W, self.H)


class Case:
    def __init__(self, name, records, Cn, N, W, H):
        self.name, self.records, self.Cn, self.N, self.W, self.H = name, records, Cn, N, W, H
        self.tw, self.th = math.ceil(W / TILE), math.ceil(H / TILE)
        r = records
        # the oracle's arrays, one entry per pair (dense = packed: it skips radius 0 itself)
        self.means2d = np.ascontiguousarray(r[:, 0:2]); self.opacities = np.ascontiguousarray(r[:, 2])
        self.conics = np.ascontiguousarray(r[:, 3:6]); self.colors = np.ascontiguousarray(r[:, 6:9])
        self.depths = np.ascontiguousarray(r[:, 9]); self.radii = np.ascontiguousarray(r[:, 10]).view(np.int32)
        self.camera_ids = (np.arange(Cn * N) // N).astype(np.int32)
        self._lists = None

    def lists(self):
        """(tiles_per_pair, sorted ids, sorted flatten ids, offsets [Cn, th, tw]) from the CPU oracle"""
        if self._lists is None:
            from oracle import gs_oracle as go
            tpg, ids, flat = go.isect_tiles(self.means2d, self.radii, self.depths, self.camera_ids, TILE, self.tw, self.th)
            ids_s, flat_s = go.sort_pairs(ids, flat)
            off = go.isect_offsets(ids_s, self.Cn, self.tw, self.th)
            self._lists = (tpg, ids_s, flat_s, off)
        return self._lists

    def tile_depths(self, off=None, n=None):
        if off is None:
            _, _, flat, off = self.lists(); n = flat.shape[0]
        o = np.append(np.asarray(off).reshape(-1), n)
        return np.diff(o).astype(int).tolist()

    def depth_colours(self):
        z = np.zeros((self.Cn * self.N, 3), np.float32); z[:, 0] = self.depths
        return z


def alpha_hit_counts(case, cell=16, first=None):
    """Independent of every rectangle rule: per (view, cell row, cell column) the number of visible records (of the first
    `first` of every view, if given) whose alpha passes 1/255 with sigma >= 0 at some pixel centre of the cell, evaluated in
    float64 like the oracle's test.  cell = 16: the least a tile list may keep; cell = 4: the cell lists of the cell forward."""
    ny, nx = math.ceil(case.H / cell), math.ceil(case.W / cell)
    out = np.zeros((case.Cn, ny, nx), int)
    px = np.arange(case.W) + 0.5; py = np.arange(case.H) + 0.5
    PX, PY = np.meshgrid(px, py)
    for k in range(case.Cn * case.N):
        if int(case.radii[k]) <= 0 or (first is not None and k % case.N >= first):
            continue
        a, b, c = (float(v) for v in case.conics[k])
        dx = float(case.means2d[k, 0]) - PX; dy = float(case.means2d[k, 1]) - PY
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        hit = (sigma >= 0) & (np.minimum(0.999, float(case.opacities[k]) * np.exp(-sigma)) >= 1.0 / 255.0)
        if cell == TILE:      # a record is only ever listed in the tiles of its reference square (gsplat's isect_tiles)
            x, y, rad = float(case.means2d[k, 0]), float(case.means2d[k, 1]), int(case.radii[k])
            inside = (np.floor(PX / 16) >= math.floor((x - rad) / 16)) & (np.floor(PX / 16) < math.ceil((x + rad) / 16)) \
                & (np.floor(PY / 16) >= math.floor((y - rad) / 16)) & (np.floor(PY / 16) < math.ceil((y + rad) / 16))
            hit &= inside
        for cy in range(ny):
            for cx in range(nx):
                if hit[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell].any():
                    out[case.camera_ids[k], cy, cx] += 1
    return out


def fused_kept_depths(case):
    """(A restatement of tight_tile_rect, constants included: it pins that the kernels keep computing what that header says,
    not that the header is right -- over-culling shows in the loss and gradient parity against the oracle's full lists, and
    test_oracle_blend.py holds alpha_hit_counts <= kept <= reference depth.)
    Per-(view, tile) list depths of the fused training path: the reference rectangle cut down to the tiles whose pixel
    centres the box around {alpha >= 1/255} reaches (tile_rect.h: tight_tile_rect), evaluated in float64.  The cases keep
    every box edge >= 0.04 px away from a pixel centre, so float32 decides alike."""
    out = np.zeros((case.Cn, case.th, case.tw), int)
    ref, tight = tile_rects(case.means2d, case.radii, case.opacities, case.conics, case.tw, case.th)
    for k in np.nonzero(case.radii > 0)[0]:
        x0, x1, y0, y1 = (int(v) for v in tight[k])
        if x1 > x0 and y1 > y0:
            out[case.camera_ids[k], y0:y1, x0:x1] += 1
    return out.reshape(-1).tolist()


def tile_rects(means2d, radii, opacities, conics, tw, th):
    """(reference rectangles, tight rectangles), each [n, 4] = x0, x1, y0, y1 in tiles, float64 evaluation of tile_rect.h:
    ref_tile_rect, and tight_tile_rect applied to it (constants included).  A pair with radius <= 0 has the empty rectangle
    (0, 0, 0, 0) in both; one whose opacity can never pass 1/255 has an empty tight rectangle.  Shared by fused_kept_depths
    and by front_cases.py, whose cases must keep tight == reference for every live pair."""
    x = np.asarray(means2d, np.float64)[:, 0]; y = np.asarray(means2d, np.float64)[:, 1]
    rad = np.asarray(radii).astype(np.float64); op = np.asarray(opacities, np.float64)
    a, b, c = (np.asarray(conics, np.float64)[:, i] for i in range(3))
    live = rad > 0

    def cl(v, hi):   # tile_clampi
        return np.where(~(v > 0), 0, np.where(v >= hi, hi, np.trunc(v))).astype(np.int64)
    x0 = cl(np.floor((x - rad) / 16), tw); x1 = cl(np.ceil((x + rad) / 16), tw)
    y0 = cl(np.floor((y - rad) / 16), th); y1 = cl(np.ceil((y + rad) / 16), th)
    ref = np.stack([x0, x1, y0, y1], 1) * live[:, None]
    vis = live & (255.0 * op > 1.0)
    with np.errstate(all="ignore"):
        det = a * c - b * b
        tau = np.log(np.where(vis, 255.0 * op, 2.0)) * (1.0002 + 4e-6 * a * c / det) + 1e-4
        ex = np.sqrt(2 * tau / det * c) * 1.0001 + 0.05; ey = np.sqrt(2 * tau / det * a) * 1.0001 + 0.05
        i64 = lambda v: np.where(vis, v, 0).astype(np.int64)
        tx0 = np.maximum(x0, np.maximum(i64(np.ceil((x - ex - 15.5) / 16)), -1))
        tx1 = np.minimum(x1, i64(np.minimum(np.floor((x + ex - 0.5) / 16), 1.0e6)) + 1)
        ty0 = np.maximum(y0, np.maximum(i64(np.ceil((y - ey - 15.5) / 16)), -1))
        ty1 = np.minimum(y1, i64(np.minimum(np.floor((y + ey - 0.5) / 16), 1.0e6)) + 1)
    tx1 = np.maximum(tx1, tx0); ty1 = np.maximum(ty1, ty0)
    tight = np.stack([tx0, tx1, ty0, ty1], 1) * vis[:, None]
    return ref, tight


# ---------------------------------------------------------------------------------------------------------------------
# float64 evaluation of the same blend (forward and analytic backward), vectorised per tile.  It follows the oracle's
# definition (gso_blend_fwd / gso_blend_bwd) term by term; the difference between the oracle's float32 pixel arithmetic
# and this one is the reference's own error, from which test_gpu_blend.py takes its gradient bounds.
def ref64(case, flat, off, v_rgb=None, v_alpha=None, colors=None, dt=np.float64):
    Cn, W, H, tw, th = case.Cn, case.W, case.H, case.tw, case.th
    m2 = case.means2d.astype(dt); con = case.conics.astype(dt)
    col = (case.colors if colors is None else colors).astype(dt); opa = case.opacities.astype(dt)
    n = m2.shape[0]
    rgb = np.zeros((Cn, H, W, 3), dt); alpha = np.zeros((Cn, H, W, 1), dt); last = np.zeros((Cn, H, W), np.int32)
    want = v_rgb is not None
    vm = np.zeros((n, 2), dt); vc = np.zeros((n, 3), dt); vcol = np.zeros((n, 3), dt); vo = np.zeros(n, dt)
    o = np.append(np.asarray(off).reshape(-1), flat.shape[0]).astype(np.int64)
    for c in range(Cn):
        for ty in range(th):
            for tx in range(tw):
                t = (c * th + ty) * tw + tx
                s, e = int(o[t]), int(o[t + 1])
                ys = np.arange(ty * 16, min(ty * 16 + 16, H)); xs = np.arange(tx * 16, min(tx * 16 + 16, W))
                if e == s:
                    continue
                ids = flat[s:e].astype(np.int64)
                PX, PY = np.meshgrid((xs + 0.5).astype(dt), (ys + 0.5).astype(dt))
                px, py = PX.reshape(-1, 1), PY.reshape(-1, 1)
                dx = m2[ids, 0][None] - px; dy = m2[ids, 1][None] - py
                A, B, Cc = con[ids, 0][None], con[ids, 1][None], con[ids, 2][None]
                sigma = dt(0.5) * (A * dx * dx + Cc * dy * dy) + B * dx * dy
                vis = np.exp(-sigma)
                ov = opa[ids][None] * vis
                a = np.minimum(dt(0.999), ov)
                valid = (sigma >= 0) & (a >= dt(1.0 / 255.0))
                a = np.where(valid, a, dt(0))
                nT = np.cumprod(1 - a, axis=1)
                stop = np.maximum.accumulate(nT <= dt(1e-4), axis=1)
                a = np.where(stop, dt(0), a)
                Tin = np.cumprod(1 - a, axis=1)
                Tex = np.concatenate([np.ones_like(Tin[:, :1]), Tin[:, :-1]], axis=1)
                w = a * Tex
                Tfin = Tin[:, -1]
                live = a > 0
                pos = np.arange(e - s)[None]
                lastk = np.where(live.any(axis=1), s + np.max(np.where(live, pos, -1), axis=1), 0)
                sel = (c, ys[:, None], xs[None, :])
                rgb[sel] = (w @ col[ids]).reshape(len(ys), len(xs), 3)
                alpha[sel] = (1 - Tfin).reshape(len(ys), len(xs), 1)
                last[sel] = lastk.reshape(len(ys), len(xs))
                if not want:
                    continue
                vr = v_rgb[sel].reshape(-1, 3).astype(dt)
                va = np.zeros(vr.shape[0], dt) if v_alpha is None else v_alpha[sel].reshape(-1).astype(dt)
                cw = w[:, :, None] * col[ids][None]                                  # [P, L, 3]
                S = np.flip(np.cumsum(np.flip(cw, 1), 1), 1) - cw                     # sum over the records behind
                ra = dt(1) / (dt(1) - a)
                v_al = ((col[ids][None] * Tex[:, :, None] - S * ra[:, :, None]) * vr[:, None, :]).sum(2)
                v_al += (Tfin * va)[:, None] * ra
                v_al = np.where(live, v_al, dt(0))
                vcol[ids] += np.einsum("pl,pc->lc", w, vr)
                pas = live & (ov <= dt(0.999))
                v_sigma = np.where(pas, -ov * v_al, dt(0))
                vc[ids, 0] += (dt(0.5) * v_sigma * dx * dx).sum(0); vc[ids, 1] += (v_sigma * dx * dy).sum(0)
                vc[ids, 2] += (dt(0.5) * v_sigma * dy * dy).sum(0)
                vm[ids, 0] += (v_sigma * (A * dx + B * dy)).sum(0); vm[ids, 1] += (v_sigma * (B * dx + Cc * dy)).sum(0)
                vo[ids] += np.where(pas, vis * v_al, dt(0)).sum(0)
    return dict(rgb=rgb, alpha=alpha, last=last, v_means2d=vm, v_conics=vc, v_colors=vcol, v_opacities=vo)


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  EXPECT[name] = (per-(view, tile) list depths, {view: saturation index local to the tile} or None)
def _depth_views(name, depths, seed):
    """one 16 x 16 view (= one tile) per entry: a list of that depth, a contributing filler at every third position and
    opacity 0 / -0.3 (present, never blended) elsewhere; no pixel saturates"""
    b = Builder(name, 16, 16, len(depths), seed)
    for c, d in enumerate(depths):
        for i in range(d):
            b.flat(c, FILL if i % 3 == 0 else (0.0 if i % 3 == 1 else -0.3))
        if d >= 3:
            b.recs[c][d // 2] = b.recs[c][d // 2][:2] + (0.3,) + b.recs[c][d // 2][3:]       # one that matters
    return b.build()


def depth_v9():
    return _depth_views("depth_v9", [0, 1, 3, 4, 5, 63, 64, 65, 0], 1)       # 9 tiles: no whole XCD round


def depth_v8():
    return _depth_views("depth_v8", [255, 256, 257, 0, 511, 512, 513, 769], 2)   # 8 tiles: one whole XCD round


SAT_AT = [13, 63, 64, 65, 255, 256, 257, 511, 512]


def sat_v9():
    """view c: SAT_AT[c] - 13 leading records that never contribute, except eight FILL ones spread among them (T stays above
    0.9), then 14 flat records of opacity 0.5 -- the 14th, at list index SAT_AT[c], saturates every pixel and is not
    blended -- and 20 live records behind it that must not be blended either"""
    b = Builder("sat_v9", 16, 16, len(SAT_AT), 3)
    for c, s in enumerate(SAT_AT):
        k = s - 13
        marks = set(np.linspace(0, k - 1, 8).astype(int).tolist()) if k >= 50 else set()
        for i in range(k):
            b.flat(c, FILL if i in marks else 0.0)
        b.flat(c, 0.5, 14)
        b.flat(c, 0.5, 10).flat(c, 0.3, 10)
    return b.build()


FSAT_AT = [255, 256, 257, 511, 512]
HARD_POS = [0, 63, 64, 255]
FSAT_FILL = 0.005       # 27 % above 1/255: survives the fused path's exact culling; 512 of them leave T = 0.077


def fsat_v5():
    """sat_v9 for the fused training path, which drops records that fail the alpha test everywhere: the leading records all
    contribute (opacity FSAT_FILL), and their number is chosen so that the n-th halving record saturates every pixel
    exactly at list index FSAT_AT[c] (float64 here; the oracle pins it)"""
    b = Builder("fsat_v5", 16, 16, len(FSAT_AT), 16)
    for c, s in enumerate(FSAT_AT):
        for k in range(s, 0, -1):
            T = (1.0 - FSAT_FILL) ** k
            n = math.ceil(math.log(1e-4 / T) / math.log(0.5))
            if k + n - 1 == s:
                break
        else:
            raise AssertionError(s)
        b.fill(c, k, other=FSAT_FILL)
        b.recs[c] = [r[:2] + (FSAT_FILL,) + r[3:] for r in b.recs[c]]
        b.flat(c, 0.5, n).flat(c, 0.4, 20)
    return b.build()


SAT_WAVE_AT = [128, 256]


def sat_wave():
    """One WAVE finished while the other three keep blending across a round / batch boundary.  View c: contributing fillers and
    halving records bring every pixel to T = 1.2e-4 at list index B - 64 (B = SAT_WAVE_AT[c]); the next 64 records are pins,
    one per pixel of quadrant 0 (view 0) / quadrant 3 (view 1), each saturating exactly its pixel: at index B - 1 the whole
    quadrant is done and no other pixel is.  The halving record at index B -- the first of the next backward round, for
    B = 256 of the next forward batch -- saturates all the others; 20 live records follow.  No opacity-0 record: the fused
    path keeps the same list."""
    b = Builder("sat_wave", 16, 16, 2, 17)
    for c, B in enumerate(SAT_WAVE_AT):
        P = B - 64
        for m in range(8, 14):
            k = P - m
            f = 1.0 - (1.2e-4 / 0.5 ** m) ** (1.0 / k)
            if 0.006 <= f <= 0.02:
                break
        else:
            raise AssertionError(B)
        for _ in range(k):
            b.flat(c, f)
        b.flat(c, 0.5, m)
        q = 0 if c == 0 else 3
        for py in range(8):
            for px in range(8):
                b.pin(c, 8 * (q & 1) + px, 8 * (q >> 1) + py)
        b.flat(c, 0.5, 1).flat(c, 0.4, 20)
    return b.build()


def fhard_v8():
    """hard_v9 for the fused path (the only way into k_blend_fwd_cells): every filler contributes (opacity FSAT_FILL), so exact
    culling keeps all 256 records of each view and the single hard record stays at position HARD_POS[c % 4] of one full
    batch: opacity 0.9985 in views 0-3, 1.2 in views 4-7"""
    b = Builder("fhard_v8", 16, 16, 8, 18)
    for c in range(8):
        for i in range(256):
            b.flat(c, (0.9985 if c < 4 else 1.2) if i == HARD_POS[c % 4] else FSAT_FILL)
    return b.build()


def xcd_v8():
    """8 views of 2 x 1 tiles: 16 workgroups = one whole round of xcd_remap with groups of two tiles, a real permutation
    (with one-tile views the remapped branch is the identity); every tile has another depth"""
    b = Builder("xcd_v8", 32, 16, 8, 19)
    for c in range(8):
        b.cflat(c, 0.05, 1, 1, c + 1).flat(c, 0.2, 1 + c % 3)
        b.sharp(c, 3 + 3 * c, 5).sharp(c, 30 - c, 9, 0.3)
    return b.build()


def sat_partial(k, name):
    """13 halving records (T = 1.22e-4), then a sharp record at pixel (3, 3) that saturates (3, 3) and (2, 3), (3, 4),
    (2, 4) ... of quadrant 0 only (alpha 0.70 / 0.26 / 0.26 / 0.09: nT 3.7e-5 / 9.1e-5 / 9.1e-5 / 1.11e-4 -- the last does
    not), then five more halving records: the first of them saturates every remaining pixel.  k leading opacity-0 records
    shift the indices: k = 242 puts the sharp record at 255 and the final one at 256."""
    b = Builder(name, 16, 16, 1, 4)
    b.fill(0, k, every=10 ** 9, other=0.0)
    b.recs[0] = [r[:2] + (0.0,) + r[3:] for r in b.recs[0]]
    b.flat(0, 0.5, 13).sharp(0, 3, 3).flat(0, 0.5, 5)
    return b.build()


def eq256():
    """37 x 21 (3 x 2 tiles, ragged right and bottom): 256 contributing fillers in every tile, nothing saturates"""
    return Builder("eq256", 37, 21, 1, 5).fill(0, 256).build()


def eq257_v2():
    b = Builder("eq257_v2", 37, 21, 2, 6).fill(0, 257)
    b.fill(1, 50).flat(1, 0.5, 14).flat(1, 0.4, 6)        # view 1: saturates at a filler-dependent index, live records behind
    return b.build()


def uneq():
    """neighbouring tiles of unequal depth (list starts that are no multiple of 64), empty tiles on the right, all depths tied
    (the order falls back to the pair id)"""
    b = Builder("uneq", 37, 21, 1, 7, tie_depths=True)
    b.cflat(0, FILL, 1, 1, 65).cflat(0, 0.1, 2, 2, 5).cflat(0, 0.3, 2, 1, 3)
    return b.build()


def cell256():
    """One batch of 256 sharp records (opacity 0.02: three-pixel footprints) that all reach cell (1, 1): 222 only that cell, 33
    also cell (0, 1), one also cell (1, 0), none cell (0, 0) -- the four lists of wave 0 are (0, 1, 33, 256) long; the other
    waves' lists are empty (test_oracle_blend.py counts them).  A second batch: three sharp records in quadrant 3 and a flat one."""
    b = Builder("cell256", 16, 16, 1, 8)
    b.sharp(0, 4, 5, 0.02, 33).sharp(0, 5, 3, 0.02, 1).sharp(0, 6, 5, 0.02, 222)
    b.sharp(0, 13, 13, 0.9, 3).flat(0, 0.3)
    return b.build()


def cell_lens():
    """cell lists whose lengths straddle 32 and 64 (the trip count is re-evaluated every 32 list positions): view 0 cells of
    quadrant 0: 31, 32, 33, 0 and of quadrant 1: 63, 64, 0, 1; view 1 quadrant 2: 65, 1, 2, 3, quadrant 3: 30, 34, 62, 0"""
    b = Builder("cell_lens", 16, 16, 2, 9)
    def cell(cam, cx, cy, n):
        b.sharp(cam, 4 * cx + 2, 4 * cy + 1, 0.02, n)
    for (cx, cy, n) in ((0, 0, 31), (1, 0, 32), (0, 1, 33), (2, 0, 63), (3, 0, 64), (3, 1, 1)):
        cell(0, cx, cy, n)
    for (cx, cy, n) in ((0, 2, 65), (1, 2, 1), (0, 3, 2), (1, 3, 3), (2, 2, 30), (3, 2, 34), (2, 3, 62)):
        cell(1, cx, cy, n)
    return b.build()


def hard_v9():
    """256 records per view, a contributing filler at every fourth position; views 0-3: one record of opacity 0.9985 (inside
    (0.998, 0.999]: not clamped, but the batch / round is no longer LEAN / easy) at position HARD_POS[c]; views 4-7: one of
    opacity 1.2 (clamped to 0.999: no gradient through it); view 8: no hard record at all"""
    b = Builder("hard_v9", 16, 16, 9, 10)
    for c in range(9):
        b.fill(c, 256, every=4, other=0.0)
        if c < 8:
            p = HARD_POS[c % 4]
            r = b.recs[c][p]
            b.recs[c][p] = r[:2] + (0.9985 if c < 4 else 1.2,) + r[3:]
    return b.build()


def needle():
    """needle conics (det < 2e-3 a c: the third cause of a hard batch) across 37 x 21, among fillers and sharp records"""
    b = Builder("needle", 37, 21, 1, 11).fill(0, 20)
    for (x, y) in ((10.3, 8.2), (25.1, 12.4), (18.7, 3.3)):
        b.add(0, x, y, 0.5, (0.05, 0.04997, 0.05), 60)
    b.sharp(0, 5, 5).sharp(0, 20, 10).fill(0, 10)
    return b.build()


def chunks():
    """Backward rounds (64 list positions) whose contributing records per wave number 1 / 2 / 3 / 5 (round 0), 1 / 63 / 0 / 0
    (round 1), 0 / 0 / 64 / 0 (round 2), 4 / 0 / 0 / 0 (round 3), then records met by 4, 2 and 3 waves, and records whose
    rectangle spans 1, 2, 4 and 6 tiles of the 3 x 2 grid while their pixels lie in tile 0.  Opacity-0 flat records pad the
    rounds."""
    b = Builder("chunks", 37, 21, 1, 12)
    b.sharp(0, 2, 2).sharp(0, 10, 2, 0.3, 2).sharp(0, 2, 10, 0.3, 3).sharp(0, 10, 10, 0.3, 5)
    b.flat(0, 0.0, 64 - 11)
    b.sharp(0, 5, 5, 0.3, 1).sharp(0, 12, 4, 0.02, 63)                        # round 1: 1 | 63
    b.sharp(0, 4, 12, 0.02, 64)                                               # round 2: wave 2
    b.sharp(0, 5, 5, 0.3, 4).flat(0, 0.0, 60)                                 # round 3: 4 of wave 0
    b.sharp(0, 7, 7).sharp(0, 7, 3).sharp(0, 7, 8)                            # 4, 2 and 3 waves
    b.sharp(0, 5, 6, 0.3).sharp(0, 14, 5, 0.3).sharp(0, 14, 14, 0.3).sharp(0, 5, 5, 0.3, radius=30)   # 1, 2, 4, 6 tiles
    b.flat(0, 0.2, 2)
    return b.build()


def gather():
    """more than 256 pairs with 0, 1, 2 and 6 slots each: 254 one-tile pairs, then a six-tile pair whose slots 254 .. 259
    cross the first 256-slot window of the gather, zero-slot pairs (radius 0, and a rectangle outside the image) in between"""
    b = Builder("gather", 37, 21, 1, 13)
    rng = np.random.default_rng(99)
    for i in range(254):
        tx, ty = i % 2, (i // 2) % 2                                          # tiles (0..1, 0..1); interior pixels only
        b.sharp(0, 16 * tx + int(rng.integers(4, 12)), (16 * ty + int(rng.integers(4, 12))) if ty == 0 else 19, 0.3)
    b.sharp(0, 5, 5, 0.3, radius=30)
    b.add(0, 400.0, 400.0, 0.5, SHARP_CONIC, 3)                               # visible radius, no tile
    b.add(0, 5.0, 5.0, 0.5, SHARP_CONIC, 0)                                   # radius 0
    b.sharp(0, 14, 5, 0.3, 20).sharp(0, 36, 20, 0.9).flat(0, 0.2, 3)
    return b.build()


def sharp300():
    """300 sharp records at random pixels of 37 x 21 under 20 flat ones: unequal tile depths, lists starting mid-word"""
    b = Builder("sharp300", 37, 21, 1, 14)
    rng = np.random.default_rng(5)
    for i in range(300):
        b.sharp(0, int(rng.integers(0, 37)), int(rng.integers(0, 21)), (0.9, 0.3, 0.02)[i % 3])
        if i % 15 == 0:
            b.flat(0, 0.1)
    return b.build()


def edge(name, W, H, Cn=1, seed=20):
    """image sizes 1, 15, 16, 17 modulo 16, 1 x 1, one row, one column: lanes outside the image start saturated and must
    neither contribute nor hold up the workgroup's break test (20 halving records: every pixel saturates at index 13 + the
    sharp ones in front of it)"""
    b = Builder(name, W, H, Cn, seed)
    for c in range(Cn):
        b.sharp(c, W - 1, H - 1).sharp(c, 0, 0, 0.3).sharp(c, W // 2, H // 2, 0.3)
        b.flat(c, 0.5, 20)
    return b.build()


def onehot16():
    """a 16 x 16 tile for the one-hot cotangent sweep: flat records and sharp ones at every cell's corners"""
    b = Builder("onehot16", 16, 16, 1, 15)
    b.flat(0, 0.2, 3)
    for cy in range(4):
        for cx in range(4):
            b.sharp(0, 4 * cx + (cx + cy) % 4, 4 * cy + (2 * cx + cy) % 4, (0.9, 0.3)[(cx + cy) % 2])
    b.flat(0, 0.3, 2)
    return b.build()


def duplicated():
    """sat_partial's records, then ALL of them once more behind full saturation: same image, zero gradient for the copies"""
    b = Builder("duplicated", 16, 16, 1, 4)
    b.flat(0, 0.5, 13).sharp(0, 3, 3).flat(0, 0.5, 5)
    b.recs[0] = b.recs[0] + list(b.recs[0])
    return b.build()


CASES = {
    "depth_v9": depth_v9, "depth_v8": depth_v8, "xcd_v8": xcd_v8, "sat_v9": sat_v9, "fsat_v5": fsat_v5,
    "sat_wave": sat_wave, "fhard_v8": fhard_v8,
    "sat_partial_0": lambda: sat_partial(0, "sat_partial_0"), "sat_partial_242": lambda: sat_partial(242, "sat_partial_242"),
    "eq256": eq256, "eq257_v2": eq257_v2, "uneq": uneq, "cell256": cell256, "cell_lens": cell_lens, "hard_v9": hard_v9,
    "needle": needle, "chunks": chunks, "gather": gather, "sharp300": sharp300, "onehot16": onehot16, "duplicated": duplicated,
    "edge_1x1": lambda: edge("edge_1x1", 1, 1), "edge_row33": lambda: edge("edge_row33", 33, 1),
    "edge_col17": lambda: edge("edge_col17", 1, 17), "edge_15": lambda: edge("edge_15", 15, 15, 2),
    "edge_17x31": lambda: edge("edge_17x31", 17, 31), "edge_32x16": lambda: edge("edge_32x16", 32, 16),
}
# the fused training call needs an SSIM window (11 x 11) inside the image
FUSED = ["xcd_v8", "sat_v9", "fsat_v5", "sat_wave", "fhard_v8", "sat_partial_242", "eq256", "eq257_v2", "uneq", "cell256", "cell_lens", "hard_v9", "needle", "chunks",
         "gather", "sharp300", "edge_15", "edge_17x31", "edge_32x16"]

_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# References, computed once per case and shared (never modified) by the tests that need them.
GRAD_KEYS = ("v_means2d", "v_conics", "v_colors", "v_opacities")
FLOOR = 5e-5            # of the tensor's maximum: the project's existing per-pair gradient bar (test_backward_vs_oracle)


def cotangents(case, seed=3):
    rng = np.random.default_rng(seed)
    v_rgb = rng.standard_normal((case.Cn, case.H, case.W, 3)).astype(np.float32)
    v_alpha = rng.standard_normal((case.Cn, case.H, case.W, 1)).astype(np.float32)
    return v_rgb, v_alpha


def oracle_bwd(case, fwd, v_rgb, v_alpha=None, colors=None):
    from oracle import gs_oracle as go
    _, _, flat, off = case.lists()
    vm, vc, vcol, vo = go.blend_bwd(case.Cn, case.W, case.H, TILE, case.means2d, case.conics,
                                    case.colors if colors is None else colors, case.opacities, off, flat, fwd["alpha"],
                                    fwd["last"], v_rgb, v_alpha)
    return dict(v_means2d=vm, v_conics=vc, v_colors=vcol, v_opacities=vo)


MED_FLOOR, P99_FLOOR = 2e-6, 1e-4       # test_backward_vs_oracle's bounds on the element-wise relative error


def grad_bounds(o32, r64):
    """per tensor: 4 x the error of the float32 evaluation of the reference itself (the oracle's float pixel arithmetic)
    against float64 on this case -- absolute with floor FLOOR x the tensor's maximum, and for the element-wise relative error
    over the elements above 1e-4 of the maximum (median, 99th percentile; floors MED_FLOOR, P99_FLOOR).  The factor 4
    covers the kernels' other grouping of the float32 sums: per 4-pixel run, per wave, then per tile slot."""
    out = {}
    for k in GRAD_KEYS:
        scale = float(np.abs(r64[k]).max())
        err = np.abs(o32[k] - r64[k])
        own = float(err.max())
        big = np.abs(o32[k]) > 1e-4 * scale
        med = p99 = 0.0
        if big.sum() >= 50:
            rel = err[big] / np.abs(o32[k][big])
            med, p99 = float(np.median(rel)), float(np.percentile(rel, 99))
        out[k] = dict(abs=max(4.0 * own, FLOOR * scale), own=own, scale=scale, big=big,
                      med=max(4.0 * med, MED_FLOOR), p99=max(4.0 * p99, P99_FLOOR))
    return out


_refs = {}


def reference(name):
    """dict: fwd (oracle rgb / alpha / last / margin), v_rgb, v_alpha, bwd[True / False] (with / without v_alpha: oracle
    gradients, float64 gradients, bounds), depth (oracle blend of (z, 0, 0) colours, its backward for v_depth, bounds)"""
    if name in _refs:
        return _refs[name]
    from oracle import gs_oracle as go
    case = get(name)
    _, _, flat, off = case.lists()
    rgb, alpha, last, margin = go.blend_fwd(case.Cn, case.W, case.H, TILE, case.means2d, case.conics, case.colors,
                                            case.opacities, off, flat, True)
    fwd = dict(rgb=rgb, alpha=alpha, last=last, margin=margin)
    v_rgb, v_alpha = cotangents(case)
    R = dict(fwd=fwd, v_rgb=v_rgb, v_alpha=v_alpha, bwd={})
    for has_va in (True, False):
        va = v_alpha if has_va else None
        o32 = oracle_bwd(case, fwd, v_rgb, va)
        r64 = ref64(case, flat, off, v_rgb, va)
        R["bwd"][has_va] = dict(o32=o32, r64=r64, bounds=grad_bounds(o32, r64))
    R["f64"] = R["bwd"][True]["r64"]
    zcol = case.depth_colours()
    d3, alpha_d, last_d, _ = go.blend_fwd(case.Cn, case.W, case.H, TILE, case.means2d, case.conics, zcol, case.opacities,
                                          off, flat)
    assert np.array_equal(alpha_d, alpha) and np.array_equal(last_d, last)
    v3 = np.zeros_like(v_rgb); v3[..., 0] = v_alpha[..., 0]                   # v_depth = v_alpha's numbers
    o32 = oracle_bwd(case, fwd, v3, None, zcol)
    r64 = ref64(case, flat, off, v3, None, zcol)
    R["depth"] = dict(d=d3[..., 0:1], v_depth=v_alpha, o32=o32, r64=r64, bounds=grad_bounds(o32, r64))
    _refs[name] = R
    return R


def fused_target(case, rgb_o, seed=7):
    """ground truth at least 0.06 (and at most 0.2) away from the oracle's render in every channel and inside [0, 1]: the
    sign of the L1 term is decided whatever the last bits of the kernel's render are"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.06, 0.2, rgb_o.shape)
    sgn = np.where(rng.random(rgb_o.shape) < 0.5, -1.0, 1.0)
    sgn = np.where(rgb_o - d < 0.0, 1.0, sgn); sgn = np.where(rgb_o + d > 1.0, -1.0, sgn)
    return (rgb_o + sgn * d).astype(np.float32)


_fused = {}


def fused_reference(name, ssim_fac=0.2):
    """oracle forward -> gradient of sum over views of (1 - ssim_fac) L1 + ssim_fac (1 - SSIM) at the oracle's render ->
    oracle blend backward (v_alpha = 0); loss, gradients, float64 gradients, bounds"""
    if name in _fused:
        return _fused[name]
    from oracle import gs_oracle as go
    case = get(name); R = reference(name)
    _, _, flat, off = case.lists()
    gt = fused_target(case, R["fwd"]["rgb"])
    loss = 0.0
    v_rgb = np.zeros_like(R["fwd"]["rgb"])
    for c in range(case.Cn):
        l1, ss, vr = go.l1_ssim(R["fwd"]["rgb"][c], gt[c], 1.0 - ssim_fac, ssim_fac)
        loss += (1.0 - ssim_fac) * l1 + ssim_fac * (1.0 - ss)
        v_rgb[c] = vr
    o32 = oracle_bwd(case, R["fwd"], v_rgb, None)
    r64 = ref64(case, flat, off, v_rgb, None)
    _fused[name] = dict(gt=gt, loss=loss, v_rgb=v_rgb, o32=o32, r64=r64, bounds=grad_bounds(o32, r64))
    return _fused[name]
