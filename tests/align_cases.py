"""Hand-built flat alignment problems for tests/test_gpu_align_cases.py (GPU) and tests/test_oracle_align_cases.py (CPU pins):
inputs, the float64 reference, the bounds and the predicates of every case.

The cases are NOT scenes: gradient parity needs no geometric consistency, so `build` draws anchors, core depths,
confidences and target pixels at random and emits the layout of st3r_synth.synth_align.flatten.  What a case plants is
the SHAPE of the work: rows per stage (wave and workgroup tails, the 32-partial hand-over to k_align_reduce, more than
1024 workgroups' worth of rows), views (LDS sizes, the 256-thread workgroup of k_align_update), the tree (root, order,
depth, branching), the clamp branches of loss_2d and of the focal, ties of min(size), the rows a core depth is read by.

Reference: oracle/align_oracle.loss_and_grads -- `Problem(flat, float64)` with torch autograd is the truth, the same code
in float32 is the yardstick.  Bounds (`group_bound`): 4 x the float32 oracle's own error against float64 on that case,
floored at 5e-5 of the group's maximum (gradients) or 1e-5 (camera table and points).  Nothing of the kernels'
arithmetic is restated here; `launch_shape` and `lds_bytes` restate the HOST formulas of st3r_align_run_opts once and
the CPU file pins them against the constants in align.hip.
"""
import functools
import math

import numpy as np
import torch

from oracle import align_oracle as ao

PARAM_KEYS = ("pps", "log_focals", "quats", "trans", "log_sizes")
WIDTH = dict(pps=2, log_focals=1, quats=4, trans=3, log_sizes=1)
# the 11 parameter groups, in the order of the Adam moments: (key, column)
GROUPS = [(k, c) for k in PARAM_KEYS for c in range(WIDTH[k])]
SIZES = [(512, 384), (384, 512), (512, 288)]      # views cycle through these: W != H, three diagonals
GRAD_FLOOR, TABLE_FLOOR, LOSS_RTOL = 5e-5, 1e-5, 2e-5
ROWS_PER_WG, MAX_WG, MAX_INLINE_PARTIALS, MAXC = 256, 1024, 32, 256


# ---------------------------------------------------------------- host formulas (pinned by the CPU file) --------------
def launch_shape(n_corr, n_c2d, n_dust, stage):
    """-> (rpt, n_part, reduce): groups of 256 rows per residual workgroup, residual workgroups of the stage, and whether
    k_align_reduce adds their partials (more than 32) instead of k_align_update"""
    max_rows = max(n_corr, n_c2d) + n_dust
    rpt = -(-(-(-max_rows // ROWS_PER_WG)) // MAX_WG) if max_rows > 0 else 1
    rows = (n_corr if stage == 1 else n_c2d) + n_dust
    n_part = -(-rows // (ROWS_PER_WG * rpt)) if rows > 0 else 0
    return rpt, n_part, n_part > MAX_INLINE_PARTIALS


def lds_bytes(C):
    """dynamic LDS of k_align_resid: four accumulator copies of 20 C + 1 floats and the camera table of 24 C"""
    return 4 * (4 * (20 * C + 1) + 24 * C)


def moment_groups(m, C):
    """[11 C] moments -> {key: [C, width]}"""
    m = np.asarray(m).reshape(-1)
    out, o = {}, 0
    for k in PARAM_KEYS:
        out[k] = m[o:o + C * WIDTH[k]].reshape(C, WIDTH[k])
        o += C * WIDTH[k]
    return out


# ---------------------------------------------------------------- builder ---------------------------------------------
def path_tree(C, root=0):
    return root, [(k, k + 1) for k in range(C - 1)]


def build(C, pairs, dust=(), pairs2d=None, tree=None, G=64, apv=48, seed=0, reserve=0):
    """C views; `pairs`: [(i, j, n)] -> n loss_3d rows (anchor of image i, anchor of image j) each, in this order;
    `pairs2d` (default: the same list) -> n loss_2d rows each (pixel in image i, anchor of image j); `dust`:
    [(i1, i2, n)] regression rows (anchor of image i1, target in the frame of i2); `tree` = (root, ordered edge list);
    every view has `apv` anchors reading `G` core depths; rows never pick the first `reserve` anchors of a view (a case
    plants rows on those itself)."""
    rng = np.random.default_rng(seed)
    imsizes = np.array([SIZES[v % 3] for v in range(C)], np.float32)
    root, edges = tree if tree is not None else path_tree(C)
    a_img = np.repeat(np.arange(C), apv)
    flat = dict(n_views=np.int64(C), imsizes=imsizes, pps=(imsizes * 0.5).astype(np.float32),
                base_focals=(560.0 * (1 + 0.1 * rng.uniform(-1, 1, C))).astype(np.float32),
                core_depth=rng.uniform(0.5, 2.0, (C, G)).astype(np.float32),
                anchor_pix=(rng.uniform(0, 1, (C * apv, 2)) * (imsizes[a_img] - 1)).astype(np.float32),
                anchor_idx=rng.integers(0, G, C * apv).astype(np.int64),
                anchor_offset=rng.uniform(0.5, 1.1, C * apv).astype(np.float32), anchor_img=a_img.astype(np.int32),
                mst_root=np.int64(root), mst_edges=np.array(edges, np.int64).reshape(-1, 2))
    pick = lambda v, n: v * apv + rng.integers(reserve, apv, n)
    conf = lambda n: rng.uniform(0.1, 1.0, n).astype(np.float32)
    cat = lambda xs, dt, shape=(0,): np.concatenate(xs).astype(dt) if len(xs) else np.zeros(shape, dt)
    pairs = [p for p in pairs if p[2] > 0]
    pairs2d = pairs if pairs2d is None else [p for p in pairs2d if p[2] > 0]
    dust = [p for p in dust if p[2] > 0]
    a1 = [pick(i, n) for i, j, n in pairs]
    # (a pair inside one image: the second anchor is another one of that image, never the same)
    a2 = [pick(j, n) if i != j else i * apv + reserve + (x - i * apv - reserve + rng.integers(1, apv - reserve, n)) % (apv - reserve)
          for (i, j, n), x in zip(pairs, a1)]
    flat.update(corr_a1=cat(a1, np.int64), corr_a2=cat(a2, np.int64),
                corr_conf=cat([conf(n) for i, j, n in pairs], np.float32))
    flat.update(c2d_pix=cat([rng.uniform(0, 1, (n, 2)) * (imsizes[i] - 1) for i, j, n in pairs2d], np.float32, (0, 2)),
                c2d_a2=cat([pick(j, n) for i, j, n in pairs2d], np.int64),
                c2d_img1=cat([np.full(n, i) for i, j, n in pairs2d], np.int32),
                c2d_conf=cat([conf(n) for i, j, n in pairs2d], np.float32))
    tgt = []
    for i1, i2, n in dust:
        z = rng.uniform(0.5, 2.0, n)
        tgt.append(np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1))
    flat.update(dust_a1=cat([pick(i1, n) for i1, i2, n in dust], np.int64), dust_tgt=cat(tgt, np.float32, (0, 3)),
                dust_img2=cat([np.full(n, i2) for i1, i2, n in dust], np.int32), dust_conf=cat([conf(n) for i1, i2, n in dust], np.float32))
    return flat


def generic_params(flat, seed):
    """a generic (non-degenerate) parameter point, like test_gpu_align._perturbed_params, around the views' own focals"""
    C = int(flat["n_views"])
    rng = np.random.default_rng(seed)
    q = np.tile(np.array([[0, 0, 0, 1.0]]), (C, 1)) + 0.1 * rng.standard_normal((C, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(pps=(0.5 + 0.02 * rng.standard_normal((C, 2))).astype(np.float32),
                log_focals=(np.log(flat["base_focals"].astype(np.float64)) + 0.05 * rng.standard_normal(C)).astype(np.float32),
                quats=q.astype(np.float32), trans=(0.2 * rng.standard_normal((C, 3))).astype(np.float32),
                log_sizes=(0.1 * rng.standard_normal(C)).astype(np.float32))


class Case:
    def __init__(self, name, flat, stage, params=None, seed=1, kw=None, expect=None, check=None, grad_floor=GRAD_FLOOR):
        self.name, self.flat, self.stage, self.grad_floor = name, flat, stage, grad_floor
        self.C = int(flat["n_views"])
        self.params = params if params is not None else generic_params(flat, seed)
        self.kw = dict(kw or {})            # options of align.run: opt_pp, gamma1, gamma2, gammad, opt_depth
        self.expect = dict(expect or {})    # what the case names: rows, n_part, rpt, ties, depth, root ... (asserted on the CPU)
        self.check = check                  # further predicate: check(case, R) with R = reference(name)

    n_corr = property(lambda s: len(s.flat["corr_a1"]))
    n_c2d = property(lambda s: len(s.flat["c2d_a2"]))
    n_dust = property(lambda s: len(s.flat["dust_a1"]))
    rows = property(lambda s: (s.n_corr if s.stage == 1 else s.n_c2d) + s.n_dust)
    shape = property(lambda s: launch_shape(s.n_corr, s.n_c2d, s.n_dust, s.stage))
    iters = property(lambda s: dict(niter1=1, niter2=0) if s.stage == 1 else dict(niter1=0, niter2=1))

    def oracle_kw(self, stage=None):
        g = self.kw.get("gamma1", 1.1) if (stage or self.stage) == 1 else self.kw.get("gamma2", 0.4)
        return dict(gamma=g, gammad=self.kw.get("gammad", 1.1))

    def trainable(self):
        """the parameter groups the stage's optimiser holds"""
        out = []
        for k, c in GROUPS:
            if k in ("quats", "trans", "log_sizes") or (self.stage == 2 and (k == "log_focals" or self.kw.get("opt_pp", True))):
                out.append((k, c))
        return out


# ---------------------------------------------------------------- reference and bounds --------------------------------
def evaluate(case, dtype, params=None, core=None, stage=None):
    return ao.loss_and_grads(case.flat, params if params is not None else case.params, stage or case.stage, dtype, core=core,
                             **case.oracle_kw(stage))


@functools.lru_cache(maxsize=None)
def reference(name):
    """{"f64": truth, "f32": yardstick} of the case at its parameter point -- computed once, never modified"""
    case = get(name)
    return {"f64": evaluate(case, torch.float64), "f32": evaluate(case, torch.float32)}


def group_bound(ref64, ref32, floor, mult=4.0):
    """-> (scale, yardstick, bound): the float32 oracle's worst error over the group's float64 maximum; bound = 4 x that,
    floored.  A group that is exactly zero in float64 has scale 0: the kernel's must be exactly zero too."""
    ref64 = np.asarray(ref64, np.float64)
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    if scale == 0.0:
        return 0.0, 0.0, floor
    yard = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) / scale
    return scale, yard, max(mult * yard, floor)


def grad_bounds(R, groups, floor=GRAD_FLOOR):
    return _grad_bounds(R, groups, floor if isinstance(floor, dict) else {}, GRAD_FLOOR if isinstance(floor, dict) else floor)


def _grad_bounds(R, groups, floors, default):
    """{(key, column): (scale, yardstick, bound)} of the reference pair R.  A group whose float64 gradient is rounding
    noise (below 1e-9 of the largest group: with one view the pose is pure gauge, its analytic gradient is zero) is
    measured against the largest group instead of against its own noise."""
    col = lambda E, k, c: E["grads"][k].reshape(-1, WIDTH[k])[:, c]
    top = max([float(np.abs(col(R["f64"], k, c)).max()) for k, c in groups] + [0.0])
    out = {}
    for k, c in groups:
        floor = floors.get((k, c), default)      # (a case may state another floor for one group: Case.grad_floor)
        scale, yard, bound = group_bound(col(R["f64"], k, c), col(R["f32"], k, c), floor)
        if 0.0 < scale < 1e-9 * top:
            yard = yard * scale / top
            scale, bound = top, max(4.0 * yard, floor)
        out[(k, c)] = (scale, yard, bound)
    return out


TABLE_KEYS = ("intrinsics", "cam2w", "depthmaps", "pts3d")


def table_bounds(R):
    return {k: group_bound(R["f64"][k], R["f32"][k], TABLE_FLOOR) for k in TABLE_KEYS}


# ---------------------------------------------------------------- per-row values of the float64 oracle ----------------
def rows3d(case, E):
    """distances of the loss_3d rows and of the regression rows in the evaluation E"""
    f, pts = case.flat, E["pts3d"]
    d = np.linalg.norm(pts[f["corr_a1"]] - pts[f["corr_a2"]], axis=-1) if case.n_corr else np.zeros(0)
    T = E["cam2w"][f["dust_img2"]] if case.n_dust else np.zeros((0, 4, 4))
    tgt = np.einsum("nij,nj->ni", T[:, :3, :3], f["dust_tgt"].astype(np.float64)) + T[:, :3, 3]
    dd = np.linalg.norm(pts[f["dust_a1"]] - tgt, axis=-1) if case.n_dust else np.zeros(0)
    return d, dd


def rows2d(case, E):
    """(rz, u, v, d) of the loss_2d rows before any clamp, from the oracle's own K, w2cam and points"""
    f = case.flat
    if not case.n_c2d:
        z = np.zeros(0)
        return z, z, z, z
    P = E["intrinsics"] @ E["w2cam"][:, :3]
    Pi = P[f["c2d_img1"]]
    r = np.einsum("nij,nj->ni", Pi[:, :, :3], E["pts3d"][f["c2d_a2"]]) + Pi[:, :, 3]
    rz = r[:, 2]
    zc = np.maximum(rz, 1e-3)
    u, v = r[:, 0] / zc, r[:, 1] / zc
    uv = np.clip(np.stack([u, v], 1), -1000, 2000)
    return rz, u, v, np.linalg.norm(f["c2d_pix"].astype(np.float64) - uv, axis=-1)


def clip_classes(rz, u, v):
    zclip = rz < 1e-3
    uclip, vclip = (u < -1000) | (u > 2000), (v < -1000) | (v > 2000)
    return dict(z=zclip, u=~zclip & uclip & ~vclip, v=~zclip & ~uclip & vclip, uv=~zclip & uclip & vclip,
                free=~zclip & ~uclip & ~vclip)


def threshold_margin(rz, u, v):
    """smallest relative distance of any row to one of the thresholds 1e-3 (rz), -1000 and 2000 (u, v)"""
    if not rz.size:
        return np.inf
    m = [np.abs(rz / 1e-3 - 1).min()]
    live = rz >= 1e-3         # (u and v of a z-clipped row are far outside or their gradient is cut anyway)
    for x in (u[live], v[live]):
        if x.size:
            m += [np.abs(x / -1000.0 - 1).min(), np.abs(x / 2000.0 - 1).min()]
    return float(min(m))


def focal_state(case):
    """(exp(log_focal) / min_focal, exp(log_focal) / max_focal) per view, float64"""
    diag = np.linalg.norm(case.flat["imsizes"].astype(np.float64), axis=1)
    fe = np.exp(case.params["log_focals"].astype(np.float64))
    return fe / (0.25 * diag), fe / (10 * diag)


def tie_count(case):
    s = np.exp(case.params["log_sizes"].astype(np.float64))
    return int((s == s.min()).sum()), float(np.sort(s)[min(int((s == s.min()).sum()), len(s) - 1)] / s.min())


def tree_depth(root, edges, C):
    """depth of the tree in edges; asserts the list is a valid chain order (every parent placed before its child)"""
    depth = {root: 0}
    for a, b in edges:
        assert a in depth and b not in depth, (a, b)
        depth[b] = depth[a] + 1
    assert len(depth) == C
    return max(depth.values())


def cameras_per_wave(case):
    """distinct cameras the 64 rows of every wave feed (stage rows: main rows, then regression rows)"""
    f = case.flat
    if case.stage == 1:
        ca, cb = f["anchor_img"][f["corr_a1"]], f["anchor_img"][f["corr_a2"]]
    else:
        ca, cb = f["c2d_img1"], f["anchor_img"][f["c2d_a2"]]
    ca = np.concatenate([ca, f["anchor_img"][f["dust_a1"]]]); cb = np.concatenate([cb, f["dust_img2"]])
    return [len(set(ca[o:o + 64]) | set(cb[o:o + 64])) for o in range(0, len(ca), 64)]


# ---------------------------------------------------------------- the cases -------------------------------------------
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def get(name):
    c = CASES[name](name)
    assert c.name == name
    return c


P3 = ((0, 1), (1, 2), (0, 2))


def split3(n, pairs=P3):
    """n rows over the three pairs of the C = 3 problems (a pair may get none)"""
    q = [n // 3 + (1 if k < n % 3 else 0) for k in range(3)]
    return [(i, j, m) for (i, j), m in zip(pairs, q)]


def _rows_case(n, stage):
    def make(name):
        return Case(name, build(3, split3(n), seed=100 + n), stage, seed=n, expect=dict(rows=n, n_dust=0))
    return make


for _n in (1, 63, 64, 65, 255, 256, 257):
    for _s in (1, 2):
        CASES[f"rows_{_n}_s{_s}"] = _rows_case(_n, _s)


def _wg_case(wg, stage):
    def make(name):
        n = 256 * (wg - 1) + 77
        return Case(name, build(3, split3(n), seed=200 + wg), stage, seed=wg, expect=dict(rows=n, n_part=wg, rpt=1, reduce=wg > 32))
    return make


for _w in (31, 32, 33, 40, 41):
    for _s in (1, 2):
        CASES[f"wg_{_w}_s{_s}"] = _wg_case(_w, _s)


@case("rpt1_262144")
def _(name):
    return Case(name, build(3, split3(262144), pairs2d=split3(500), seed=31), 1, seed=31,
                expect=dict(rows=262144, n_part=1024, rpt=1, reduce=True))


@case("rpt2_262145")
def _(name):   # 513 workgroups of 512 rows, the last one holds one row
    return Case(name, build(3, split3(262145), pairs2d=split3(500), seed=32), 1, seed=32,
                expect=dict(rows=262145, n_part=513, rpt=2, reduce=True))


@functools.lru_cache(maxsize=None)
def _uneven_flat():
    return build(3, split3(300000), pairs2d=split3(5000), seed=33)


@case("uneven_300000_5000_s1")
def _(name):
    return Case(name, _uneven_flat(), 1, seed=33, expect=dict(rows=300000, n_part=586, rpt=2, reduce=True))


@case("uneven_300000_5000_s2")
def _(name):   # rpt = 2 comes from the OTHER stage's rows: 5000 rows in 10 workgroups of 512
    return Case(name, _uneven_flat(), 2, seed=33, expect=dict(rows=5000, n_part=10, rpt=2, reduce=False))


def _tail_case(rem, stage):
    def make(name):   # main rows % 64 = rem, then regression rows: (rem != 0) one wave holds rows of both kinds
        n = 128 + rem
        return Case(name, build(3, split3(n), dust=[(2, 0, 60), (1, 0, 40)], seed=300 + rem), stage, seed=rem + 7,
                    expect=dict(rows=n + 100, n_main=n, n_dust=100))
    return make


for _r in (0, 1, 63):
    for _s in (1, 2):
        CASES[f"tail_main{_r}_dust_s{_s}"] = _tail_case(_r, _s)


def _dust_only(stage):
    def make(name):
        return Case(name, build(3, [], dust=[(2, 0, 70), (1, 0, 50), (0, 2, 30)], seed=41), stage, seed=41,
                    expect=dict(rows=150, n_main=0, n_dust=150))
    return make


def _no_rows(stage):
    def make(name):
        return Case(name, build(3, [], seed=42), stage, seed=42, expect=dict(rows=0, n_part=0, n_main=0, n_dust=0))
    return make


for _s in (1, 2):
    CASES[f"dust_only_s{_s}"] = _dust_only(_s)
    CASES[f"no_rows_s{_s}"] = _no_rows(_s)


def _wave_mix(stage):
    def make(name):   # four waves whose 64 rows feed 1, 2, 3 and 6 cameras; the first wave's pairs lie in ONE image
        pairs = [(0, 0, 64), (0, 1, 64), (0, 1, 32), (1, 2, 32), (0, 1, 22), (2, 3, 21), (4, 5, 21)]
        return Case(name, build(6, pairs, seed=43), stage, seed=43, expect=dict(rows=256, cams_per_wave=[1, 2, 3, 6]))
    return make


for _s in (1, 2):
    CASES[f"wave_mix_s{_s}"] = _wave_mix(_s)


SAME_ANCHOR_ROWS = (0, 100, 191)


@case("same_anchor_s1")
def _(name):   # rows with a1 == a2: d == 0 exactly, no gradient from them on either side, rho(0) = 0 in the loss
    flat = build(3, split3(192), seed=44)
    for r in SAME_ANCHOR_ROWS:
        flat["corr_a2"][r] = flat["corr_a1"][r]

    def check(c, R):
        d, _ = rows3d(c, R["f64"])
        assert (d[list(SAME_ANCHOR_ROWS)] == 0).all() and (np.delete(d, SAME_ANCHOR_ROWS) > 1e-3).all()
    return Case(name, flat, 1, seed=44, expect=dict(rows=192, zero_rows=3), check=check)


def sparse_pairs(C, edges, seed, chords=8):
    """the tree's edges plus a few chords, 40 .. 70 rows per pair: most waves mix cameras"""
    rng = np.random.default_rng(seed)
    pairs = [(a, b, int(rng.integers(40, 71))) for a, b in edges]
    for _ in range(min(chords, C * (C - 1) // 2 - len(edges)) if C > 2 else 0):
        a, b = rng.choice(C, 2, replace=False)
        pairs.append((int(a), int(b), int(rng.integers(40, 71))))
    return pairs


# Seeds: a draw is replaced by the next one when, in the float64 oracle, a loss_2d row comes within 1e-3 of a clamp
# threshold, or is so close to its camera's plane (rz of a few 1e-3 with one coordinate still unclipped) that float32
# autograd of the oracle itself is off by more than 5e-4 of a group (4 x that is the 2e-3 of the older gradient checks).
# The CPU file asserts both: the margin of 1e-3, and bound = 4 x yardstick <= 2e-3 (one case states another cap).
RESEED = {("views", 63): 1, ("views", 65): 4, ("pathrev", 64): 2, ("mid", 64): 2, ("bfs", 64): 1}


def _views_case(C, stage):
    def make(name):
        root, edges = path_tree(C)
        k = 500 + C + 1000 * RESEED.get(("views", C), 0)
        flat = build(C, sparse_pairs(C, edges, k), tree=(root, edges), seed=k)
        # The one stated exception to the floor of 5e-5: stage 2 on the two 255-edge chains has a floor of 2.6e-4 (255
        # views) and 4.3e-4 (256 views) on every group.  The float32 oracle's own error is not a stable yardstick there:
        # the same code on the same inputs gives, depending on the CPU, 1.5e-5 .. 6.5e-5 on the log-focal group (255
        # views) and 2.6e-5 .. 5.6e-5 (256 views), whatever the row order or the thread count; which group its largest
        # error lands in differs too (quats[2] at 256 views: 1.07e-4), and none of 48 draws kept it under the floor.  The
        # floors are 4 x the largest figure the float32 oracle has shown on any group of the case.  Under the rule alone
        # the kernels miss on log_focals, trans[2] and log_sizes, by 4 .. 30 %.
        deep2 = stage == 2 and C >= 255
        return Case(name, flat, stage, seed=k - 500, expect=dict(views=C, big_lds=lds_bytes(C) > 64 * 1024, depth=C - 1, root=0),
                    grad_floor={255: 2.6e-4, 256: 4.3e-4}[C] if deep2 else GRAD_FLOOR)
    return make


for _c in (1, 2, 63, 64, 65, 157, 158, 255, 256):
    for _s in (1, 2):
        CASES[f"views_c{_c}_s{_s}"] = _views_case(_c, _s)


def binary_edges(C):
    return [((k - 1) // 2, k) for k in range(1, C)]


def tree_of(kind, C):
    """-> (root, ordered edges, depth the kind names)"""
    if kind == "path0":
        return 0, [(k, k + 1) for k in range(C - 1)], C - 1
    if kind == "pathrev":     # the same path rooted at its other end: every child below its parent
        return C - 1, [(k, k - 1) for k in range(C - 1, 0, -1)], C - 1
    if kind == "mid":         # root in the middle, the two arms listed alternately
        m, e = C // 2, []
        for k in range(1, C):
            if m + k < C:
                e.append((m + k - 1, m + k))
            if m - k >= 0:
                e.append((m - k + 1, m - k))
        return m, e, max(m, C - 1 - m)
    if kind == "star":
        return 2, [(2, k) for k in range(C) if k != 2], 1
    depth = int(math.floor(math.log2(C)))
    if kind == "bfs":
        return 0, binary_edges(C), depth
    if kind == "shuffled":    # the binary tree under a random relabelling, listed depth first: sorted by neither index
        perm = np.random.default_rng(C).permutation(C)
        kids = {}
        for a, b in binary_edges(C):
            kids.setdefault(a, []).append(b)
        e, stack = [], [0]
        while stack:
            a = stack.pop()
            for b in kids.get(a, []):
                e.append((int(perm[a]), int(perm[b])))
                stack.append(b)
        return int(perm[0]), e, depth
    raise KeyError(kind)


TREE_KINDS = ("path0", "pathrev", "mid", "star", "bfs", "shuffled")


def _tree_case(kind, C, stage):
    def make(name):
        root, edges, depth = tree_of(kind, C)
        k = 600 + C + 1000 * RESEED.get((kind, C), 0)
        flat = build(C, sparse_pairs(C, edges, k), tree=(root, edges), seed=k)

        def check(c, R):
            e = np.array(edges)
            if kind == "shuffled":
                assert root != 0 and (np.diff(e[:, 0]) < 0).any() and (np.diff(e[:, 1]) < 0).any() and (e[:, 1] < e[:, 0]).any()
            if kind == "pathrev":
                assert (e[:, 1] < e[:, 0]).all()
        return Case(name, flat, stage, seed=k - 599, expect=dict(root=root, depth=depth), check=check)
    return make


for _k in TREE_KINDS:
    for _c in (9, 64):
        for _s in (1, 2):
            CASES[f"tree_{_k}_c{_c}_s{_s}"] = _tree_case(_k, _c, _s)


# ---- clamps (stage 2, C = 4, a star so that the planted poses do not chain) ----
STAR4 = (0, [(0, 1), (0, 2), (0, 3)])
ALL_PAIRS4 = [(i, j, 60) for i in range(4) for j in range(4) if i != j]


def clamp_params(flat, seed):
    """generic, with view 2 turned by about pi about y and views 1 and 3 far to the side (x resp. y and x)"""
    p = generic_params(flat, seed)
    q = np.array([0.05, 1.0, -0.04, 0.06]); p["quats"][2] = (q / np.linalg.norm(q)).astype(np.float32)
    p["trans"][1] += np.array([2.2, 0.1, 0.0], np.float32)
    p["trans"][3] += np.array([0.9, 2.0, 0.1], np.float32)
    return p


def plant_behind_plane(flat, params, cam, n, seed):
    """Appends n anchors and n loss_2d rows of camera `cam` whose point lies BEHIND that camera's plane (rz < 1e-3)
    yet reprojects inside [-1000, 2000]: u = rx / 1e-3 needs |f qx + cx qz| of about 1e-3 x a pixel coordinate, which no
    random draw gives (a row behind the plane is otherwise clipped in u and v too, and the zclip branch multiplies
    zeros).  The anchor (image, pixel, offset) is solved from the float64 oracle's own cameras at `params`."""
    rng = np.random.default_rng(seed)
    E = ao.loss_and_grads(flat, params, 2, torch.float64)
    K, T, depth = E["intrinsics"], E["cam2w"], E["depthmaps"]
    C, G = int(flat["n_views"]), flat["core_depth"].shape[1]
    out = []
    for _ in range(100000):
        if len(out) == n:
            break
        u, v = rng.uniform(-600, 1600, 2)                       # where the row reprojects
        qz = -rng.uniform(0.2, 2.0)
        r = np.array([u * 1e-3, v * 1e-3, qz])                  # K q, with the clamped rz = 1e-3 dividing
        q = np.linalg.solve(K[cam], r)
        pw = T[cam, :3, :3] @ q + T[cam, :3, 3]
        j = int(rng.choice([x for x in range(C) if x != cam]))
        pc = T[j, :3, :3].T @ (pw - T[j, :3, 3])
        if pc[2] <= 0.2:
            continue
        pix = K[j, :2, :2] @ (pc[:2] / pc[2]) + K[j, :2, 2]
        idx = int(rng.integers(0, G))
        off = 1 + (pc[2] / depth[j, idx] - 1) * K[j, 0, 0] / float(flat["base_focals"][j])
        if (pix < 1).any() or (pix > flat["imsizes"][j] - 2).any() or not 0.52 <= off <= 1.08:
            continue
        out.append((j, pix, idx, off, rng.uniform(0, 1, 2) * (flat["imsizes"][cam] - 1), rng.uniform(0.1, 1.0)))
    assert len(out) == n
    A = len(flat["anchor_idx"])
    app = lambda k, x, dt: np.concatenate([flat[k], np.asarray(x, dt).reshape((-1,) + flat[k].shape[1:])]).astype(dt)
    flat["anchor_img"] = app("anchor_img", [o[0] for o in out], np.int32)
    flat["anchor_pix"] = app("anchor_pix", [o[1] for o in out], np.float32)
    flat["anchor_idx"] = app("anchor_idx", [o[2] for o in out], np.int64)
    flat["anchor_offset"] = app("anchor_offset", [o[3] for o in out], np.float32)
    flat["c2d_a2"] = app("c2d_a2", A + np.arange(n), np.int64)
    flat["c2d_img1"] = app("c2d_img1", [cam] * n, np.int32)
    flat["c2d_pix"] = app("c2d_pix", [o[4] for o in out], np.float32)
    flat["c2d_conf"] = app("c2d_conf", [o[5] for o in out], np.float32)
    return flat


@case("clamp_uvz_s2")
def _(name):
    flat = build(4, ALL_PAIRS4, tree=STAR4, seed=51)

    def check(c, R):
        cl = clip_classes(*rows2d(c, R["f64"])[:3])
        counts = {k: int(v.sum()) for k, v in cl.items()}
        assert min(counts[k] for k in ("z", "u", "v", "uv")) >= 8, counts
        per_cam = np.bincount(c.flat["c2d_img1"][cl["free"]], minlength=4)
        assert per_cam.min() >= 8, per_cam
    return Case(name, flat, 2, params=clamp_params(flat, 51), expect=dict(rows=720), check=check)


@case("clamp_behind_s2")
def _(name):
    """the zclip branch with something to zero: in `clamp_uvz_s2` every row behind the plane is clipped in u and v as
    well.  Dividing by the clamped 1e-3 amplifies float32 rounding a thousandfold, and the float32 ORACLE is off by 4e-3
    of a group here: the case's bound is 4 x that, by the rule, and says so (`max_bound`); what it is for -- a gradient
    through rz that must be cut -- is 500 times the whole gradient."""
    flat = build(4, ALL_PAIRS4, tree=STAR4, seed=51)
    params = clamp_params(flat, 51)
    flat = plant_behind_plane(flat, params, 2, 8, 51)

    def check(c, R):
        rz, u, v, d = rows2d(c, R["f64"])
        cl = clip_classes(rz, u, v)
        inside = cl["z"] & (u > -800) & (u < 1800) & (v > -800) & (v < 1800)
        assert int(inside.sum()) == 8 and inside[-8:].all() and (rz[-8:] < -0.1).all()
    return Case(name, flat, 2, params=params, expect=dict(rows=728, max_bound=5e-2), check=check)


def focal_clamp_params(flat, seed):
    p = generic_params(flat, seed)
    diag = np.linalg.norm(flat["imsizes"].astype(np.float64), axis=1)
    p["log_focals"][1] = np.float32(np.log(0.2 * diag[1])); p["log_focals"][2] = np.float32(np.log(11 * diag[2]))
    return p


def _focal_clamp(stage):
    def make(name):
        flat = build(4, ALL_PAIRS4, tree=STAR4, seed=52)

        def check(c, R):
            lo, hi = focal_state(c)
            assert lo[1] < 1 and hi[2] > 1 and (np.delete(lo, 1) > 1 + 1e-3).all() and (np.delete(hi, 2) < 1 - 1e-3).all()
            g = R["f64"]["grads"]["log_focals"]
            diag = np.linalg.norm(c.flat["imsizes"].astype(np.float64), axis=1)
            assert g[1] == 0 and g[2] == 0 and (c.stage == 1 or (g[[0, 3]] != 0).all())
            K = R["f64"]["intrinsics"]
            assert K[1, 0, 0] == 0.25 * diag[1] and K[2, 0, 0] == 10 * diag[2]
        return Case(name, flat, stage, params=focal_clamp_params(flat, 52), expect=dict(fclip=[1, 2]), check=check)
    return make


for _s in (1, 2):
    CASES[f"focal_clamp_s{_s}"] = _focal_clamp(_s)


@case("opt_pp_off_s2")
def _(name):
    return Case(name, build(4, ALL_PAIRS4, dust=[(3, 0, 40)], tree=STAR4, seed=53), 2, seed=53, kw=dict(opt_pp=False))


@case("gamma1_loss1_s1")
def _(name):
    return Case(name, build(4, ALL_PAIRS4, dust=[(3, 0, 40)], tree=STAR4, seed=54), 1, seed=54, kw=dict(gamma1=1.0))


@case("gamma1_loss2_s2")
def _(name):
    return Case(name, build(4, ALL_PAIRS4, dust=[(3, 0, 40)], tree=STAR4, seed=55), 2, seed=55, kw=dict(gamma2=1.0))


@case("gamma1_lossd_s1")
def _(name):
    return Case(name, build(4, ALL_PAIRS4, dust=[(3, 0, 40), (1, 2, 50)], tree=STAR4, seed=56), 1, seed=56, kw=dict(gammad=1.0))


@case("gamma1_lossd_s2")
def _(name):
    return Case(name, build(4, ALL_PAIRS4, dust=[(3, 0, 40), (1, 2, 50)], tree=STAR4, seed=57), 2, seed=57, kw=dict(gammad=1.0))


# ---- ties of min(size) (C = 5) ----
TIES = dict(unique=([0.3, -0.2, 0.1, -0.15, 0.25], 1), two=([0.3, -0.2, 0.1, -0.2, 0.25], 2), all=([0.05] * 5, 5))


def _tie_case(kind, stage):
    def make(name):
        root, edges, _ = tree_of("bfs", 5)
        flat = build(5, sparse_pairs(5, edges, 61, chords=4), dust=[(4, 0, 30)], tree=(root, edges), seed=61)
        p = generic_params(flat, 61)
        p["log_sizes"] = np.array(TIES[kind][0], np.float32)
        return Case(name, flat, stage, params=p, expect=dict(ties=TIES[kind][1]))
    return make


for _k in TIES:
    for _s in (1, 2):
        CASES[f"tie_{_k}_s{_s}"] = _tie_case(_k, _s)


# ---- opt_depth: the rows a core depth is read by ----
def _depth_case(C, G, planted):
    def make(name):
        pairs = [] if C == 1 else [(i, j, 50) for i in range(C) for j in range(C) if i != j][:8]
        # (one view: a loss_2d row would reproject a point into its own image, whatever the parameters -- its analytic
        # gradient is zero and both sides would compare rounding noise; regression rows have free targets)
        dust = [(0, 0, 270)] if C == 1 else [(1, 0, 30), (0, 2, 30)]
        flat = build(C, pairs, dust=dust, G=G, apv=24, seed=70 + C, reserve=5 if planted else 0)
        exp = dict(elems=C * G)
        if planted:
            # view 0: core depth 5 read by 1 row, 6 by 2 rows, 7 by 300 rows, 8 by none, 9 through TWO anchors (3 + 2 rows)
            idx = flat["anchor_idx"]
            idx[(flat["anchor_img"] == 0) & (idx >= 5) & (idx <= 9)] = 11
            idx[0:5] = [5, 6, 7, 9, 9]
            extra = np.repeat(np.arange(5), [1, 2, 300, 3, 2])
            rng = np.random.default_rng(7)
            img1 = rng.integers(1, C, len(extra))
            flat["c2d_a2"] = np.concatenate([flat["c2d_a2"], extra]).astype(np.int64)
            flat["c2d_img1"] = np.concatenate([flat["c2d_img1"], img1]).astype(np.int32)
            flat["c2d_pix"] = np.concatenate([flat["c2d_pix"], rng.uniform(0, 1, (len(extra), 2)) * (flat["imsizes"][img1] - 1)]).astype(np.float32)
            flat["c2d_conf"] = np.concatenate([flat["c2d_conf"], rng.uniform(0.1, 1, len(extra))]).astype(np.float32)
            exp["reads_view0"] = {5: 1, 6: 2, 7: 300, 8: 0, 9: 5}
        return Case(name, flat, 2, seed=70 + C, kw=dict(opt_depth=True), expect=exp)
    return make


CASES["depth_planted_255"] = _depth_case(3, 85, True)
CASES["depth_256"] = _depth_case(4, 64, False)
CASES["depth_257"] = _depth_case(1, 257, False)


def depth_reads(case):
    """rows of stage 2 (loss_2d rows, then regression rows) per core depth [C, G]"""
    f = case.flat
    a = np.concatenate([f["c2d_a2"], f["dust_a1"]])
    G = f["core_depth"].shape[1]
    return np.bincount(f["anchor_img"][a].astype(np.int64) * G + f["anchor_idx"][a], minlength=case.C * G).reshape(case.C, G)


# ---- second step / stage change / NaN stop: problems (the runs are in the GPU file) ----
@case("steps_2000")
def _(name):
    return Case(name, build(4, [(i, j, 167) for i in range(4) for j in range(4) if i != j], dust=[(3, 0, 40)],
                            tree=(1, [(1, 0), (1, 2), (2, 3)]), seed=81), 1, seed=81, expect=dict(n_part=8))


@case("steps_33wg")
def _(name):
    return Case(name, build(4, [(i, j, 700) for i in range(4) for j in range(4) if i != j], dust=[(3, 0, 40)],
                            tree=(1, [(1, 0), (1, 2), (2, 3)]), seed=82), 1, seed=82, expect=dict(n_part=33, reduce=True))


@case("steps_depth")
def _(name):
    return Case(name, build(4, [(i, j, 167) for i in range(4) for j in range(4) if i != j], dust=[(3, 0, 40)],
                            tree=(1, [(1, 0), (1, 2), (2, 3)]), apv=24, seed=83), 2, seed=83, kw=dict(opt_depth=True))


def nan_case(wgs, stage):
    """a clean problem of `wgs` residual workgroups and the same with one NaN planted (a loss_2d target pixel in stage
    2, a loss_3d confidence -- hence every weight -- in stage 1)"""
    n = 256 * (wgs - 1) + 40
    clean = build(3, split3(n), seed=90 + wgs)
    bad = {k: np.array(v, copy=True) for k, v in clean.items()}
    if stage == 2:
        bad["c2d_pix"][n // 2, 0] = np.nan
    else:
        bad["corr_conf"][n // 2] = np.nan
    assert launch_shape(n, n, 0, stage)[1] == wgs
    return clean, bad, generic_params(clean, 90 + wgs)


STEP_CASES = ("steps_2000", "steps_33wg", "steps_depth")
# the cases that are ONE call each (loss, gradients, table, points)
SINGLE = [n for n in CASES if n not in STEP_CASES]
