"""A catalogue of CALLS for the context-history suite (test_gpu_history.py; the CPU pins are in
test_oracle_history_cases.py).  Importing this module needs neither torch nor a GPU.

The property under test: the outputs of a call are a function of its arguments, the registrations, the debug flags and the
chunk count of the context -- never of what the context ran before.  So every call here has

    name          "<entry point>:<inputs>"
    kind          "train" (st3r_gs_train_fwd_bwd / _step / _step_poses: walks its views in the context's chunks), else "other"
    views         C of a training call (a chunk count is clamped to it; one view never makes the count stick)
    run(ctx)      -> {output name: tensor}, through `ops`.  The buffers a call hands over itself (gradients, losses,
                  v_records, v_viewmats, v_exposure, v_Ks) are NaN before the call; the outputs that `ops`, `matching` and
                  `align` allocate themselves with torch.empty / torch.empty_like (images, alpha, depth, last_ids, sorted
                  keys, scans, peeks ...) are poisoned by the runner, which runs every call under
                  test_gpu_history.poisoned_allocations -- without it the caching allocator would hand such a call the
                  block that still holds the result of its own previous run

and its inputs are FIXED: built once from the existing scene builders and case modules (st3r_synth.synth.make_scene with
the TRAIN_SCENES parameters of test_gpu_blend.py, blend_cases, mcmc_cases, condense_cases, dense_cases, loss_mask_cases,
align_cases), cached on the device, and never written -- a call that updates parameters in place works on clones.  No
input of a call depends on the output of another call, so the same call gives the same bits wherever it stands in a history.

Fused scenes (N, views, W, H, seed, scale_lo, scale_hi), counts from the oracle (test_oracle_history_cases.py):
  regular/a, /b   8000 x 3, 96 x 64    ~43 000 records, 0.22 of 8 N C: no TOUCH.  TRAIN_SCENES["regular"] with 8000
                                       Gaussians instead of 400: at 400 (2 100 records) the backward writes 97 % of its
                                       slots and only 5 % of a seed's pairs own a slot that the other seed alone writes;
                                       at 8000 the tiles saturate, a quarter of the slots stays unwritten, 24 % of the pairs
  large/a, /b     300 x 2, 160 x 96    ~9 800 records, 2.0 x 8 N C: k_blend_bwd<false, true>; 81 % of the pairs
  dense_small     6000 x 2, 160 x 96   ~28 700 records, 0.3 of 8 N C: no TOUCH, and more than any slot capacity that a
                                       `large` call leaves behind (x 1.25 twice: the asynchronous hint, then the arena)
  one_view, four_views                 TRAIN_SCENES["regular"] as it is (400) on 1 and 4 cameras (view chunks clamped to C)
The second seed of a scene has the same (N, C, W, H): the arena does not grow, the hint signature is the same, and the
slot layout (`cum`) is another one.
"""
import math

import numpy as np

F = np.float32

SCENES = {
    # name: (N, views, W, H, seed, scale_lo, scale_hi)
    "regular/a": (8000, 3, 96, 64, 7, 0.01, 0.08),           # test_gpu_blend.py: TRAIN_SCENES["regular"], more Gaussians
    "regular/b": (8000, 3, 96, 64, 107, 0.01, 0.08),
    "large/a": (300, 2, 160, 96, 31, 0.15, 0.3),             # TRAIN_SCENES["large"]
    "large/b": (300, 2, 160, 96, 131, 0.15, 0.3),
    "dense_small": (6000, 2, 160, 96, 5, 0.02, 0.06),
    "one_view": (400, 1, 96, 64, 7, 0.01, 0.08),
    "four_views": (400, 4, 96, 64, 7, 0.01, 0.08),
}
# the oracle's record counts (test_oracle_history_cases.py asserts them equal to history_cases.records): the GPU file
# compares the calls' statistics with these and does no oracle work
RECORDS = {"regular/a": 43156, "regular/b": 43281, "large/a": 9862, "large/b": 9614, "dense_small": 28700}
TOUCH = {"regular/a": False, "regular/b": False, "large/a": True, "large/b": True, "dense_small": False,
         "one_view": False, "four_views": False}
PAIRS = (("regular/a", "regular/b"), ("large/a", "large/b"))
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
DEPTH_FAC, ALPHA_FAC = 0.5, 0.5
SORT_TILE = 4096          # items of one tile of the radix sort at these sizes (test_gpu_sort.py: SIZES)
GROW = lambda n: (n + n // 4 + 255) & ~255          # st3r_arena_get2 on bytes; monotone, so it orders record counts alike

_scenes, _slots = {}, {}


def scene(name):
    """numpy inputs of a fused scene: Gaussians, cameras, a ground truth, a depth prior and its weights"""
    if name not in _scenes:
        from st3r_synth import synth
        N, V, W, H, seed, lo, hi = SCENES[name]
        g, w2c, Ks = synth.make_scene(N, V, W, H, seed=seed, scale_lo=lo, scale_hi=hi)
        rng = np.random.default_rng(1000 + seed)
        s = dict(N=N, V=V, W=W, H=H, w2c=w2c.astype(F), Ks=Ks.astype(F),
                 campos=np.linalg.inv(w2c.astype(np.float64))[:, :3, 3].astype(F),
                 P={k: np.ascontiguousarray(g[k], F) for k in ("means", "quats", "scales", "opacities", "shN")},
                 gt=rng.uniform(0, 1, (V, H, W, 3)).astype(F),
                 prior=rng.uniform(2.0, 5.0, (V, H, W)).astype(F), prior_w=rng.uniform(0, 1, (V, H, W)).astype(F))
        _scenes[name] = s
    return _scenes[name]


# ---- what the oracle says about a fused scene (CPU) ----
def scene_slots(name):
    """(cum [N * C] inclusive, written [n_records] bool): the slot layout of the fused path -- a pair's slots are the tiles
    of its tight rectangle (blend_cases.tile_rects, the restatement of tight_tile_rect), in pair-id order -- and, per slot,
    whether the backward writes it: the record passes alpha >= 1/255 on a pixel of the tile that is not yet saturated
    (T > 1e-4 after it), float64, records in (depth, pair id) order."""
    if name in _slots:
        return _slots[name]
    from oracle import gs_oracle as go
    import blend_cases as bc
    s = scene(name)
    N, V, W, H = s["N"], s["V"], s["W"], s["H"]
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    p = go.project_packed(s["P"]["means"], s["P"]["quats"], s["P"]["scales"], s["w2c"], s["Ks"], W, H)
    op = s["P"]["opacities"][p["gaussian_ids"]].astype(np.float64)
    _, tight = bc.tile_rects(p["means2d"], p["radii"], op, p["conics"], tw, th)
    pid = p["camera_ids"].astype(np.int64) * N + p["gaussian_ids"]
    per_pair = np.zeros(N * V, np.int64)
    per_pair[pid] = (tight[:, 1] - tight[:, 0]) * (tight[:, 3] - tight[:, 2])
    cum = np.cumsum(per_pair)
    base = cum - per_pair
    written = np.zeros(int(cum[-1]), bool)
    order = np.lexsort((pid, p["depths"]))
    py, px = np.mgrid[0:16, 0:16]
    for c in range(V):
        mine = order[p["camera_ids"][order] == c]
        for ty in range(th):
            for tx in range(tw):
                k = mine[(tight[mine, 0] <= tx) & (tx < tight[mine, 1]) & (tight[mine, 2] <= ty) & (ty < tight[mine, 3])]
                if not len(k):
                    continue
                X = (16 * tx + px + 0.5)[None]; Y = (16 * ty + py + 0.5)[None]
                inside = ((16 * tx + px < W) & (16 * ty + py < H))[None]
                dx = p["means2d"][k, 0].astype(np.float64)[:, None, None] - X
                dy = p["means2d"][k, 1].astype(np.float64)[:, None, None] - Y
                a, b, cc = (p["conics"][k, i].astype(np.float64)[:, None, None] for i in range(3))
                sigma = 0.5 * (a * dx * dx + cc * dy * dy) + b * dx * dy
                alpha = np.minimum(0.999, op[k][:, None, None] * np.exp(-sigma))
                hit = inside & (sigma >= 0) & (alpha >= 1.0 / 255.0)
                T = np.cumprod(np.where(hit, 1.0 - alpha, 1.0), 0)
                contributes = hit & (T > 1e-4)
                slot = base[pid[k]] + (ty - tight[k, 2]) * (tight[k, 1] - tight[k, 0]) + (tx - tight[k, 0])
                written[slot] = contributes.reshape(len(k), -1).any(1)
    _slots[name] = (cum, written)
    return cum, written


def records(name):
    return int(scene_slots(name)[0][-1])


def stale_pairs(mine, other):
    """the fraction of `mine`'s slot-owning pairs that own a slot which `other` writes and `mine` does not: what a call on
    `mine` after a call on `other` reads stale"""
    cum, w = scene_slots(mine)
    _, wo = scene_slots(other)
    n = min(len(w), len(wo))
    stale = np.zeros(len(w), bool)
    stale[:n] = wo[:n] & ~w[:n]
    first = np.concatenate([[0], cum[:-1]])
    owns = cum > first
    c = np.concatenate([[0], np.cumsum(stale)])
    return float(((c[cum] - c[first]) > 0).sum()) / float(owns.sum())


# ---- device side ----
_dev = {}


def on_device(key, build):
    """inputs of a call on the GPU, made once and never written"""
    if key not in _dev:
        import torch
        put = lambda a: a if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda:0")
        made = build()
        _dev[key] = {k: ({j: put(w) for j, w in v.items()} if isinstance(v, dict) else put(v)) for k, v in made.items()}
    return _dev[key]


def nan(shape):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), device="cuda:0")


def dscene(name):
    s = scene(name)
    return on_device(("scene", name), lambda: {k: s[k] for k in ("w2c", "Ks", "campos", "P", "gt", "prior", "prior_w")})


class Call:
    def __init__(self, name, run, kind="other", views=0, scene=None):
        self.name, self.run, self.kind, self.views, self.scene = name, run, kind, views, scene


def _fwd_bwd(sc, stats=True):
    def run(ctx):
        from starst3r_amd import ops
        s, d = scene(sc), dscene(sc)
        grads, loss = nan(23 * s["N"]), nan(1)
        st = ops.train_fwd_bwd(ctx, d["P"], d["w2c"], d["Ks"], d["campos"], d["gt"], s["W"], s["H"], 0.2, 0.01, 0.01, grads,
                               loss, want_stats=stats)
        out = dict(grads=grads, loss=loss)
        if stats:
            out["_n_isects"] = st["n_isects"]
        return out
    return run


def _steps(sc, n=3):
    """n consecutive train_step calls without statistics: on a fresh context the first sizes its buffers exactly, the others
    run on the record-count hint; in a history the first may find a hint of the same (N, C, W, H)"""
    def run(ctx):
        import torch
        from starst3r_amd import ops
        s, d = scene(sc), dscene(sc)
        P = {k: v.clone() for k, v in d["P"].items()}
        grads, losses = nan(23 * s["N"]), nan(n)
        m, v = torch.zeros_like(grads), torch.zeros_like(grads)
        for it in range(n):
            ops.train_step(ctx, P, d["w2c"], d["Ks"], d["campos"], d["gt"], s["W"], s["H"], 0.2, 0.01, 0.01, grads, m, v, LR,
                           B1, B2, EPS, it + 1, losses[it:it + 1], want_stats=False)
        return dict(grads=grads, losses=losses, m=m, v=v, **P)
    return run


def _poses(sc, prior, everything=False):
    """train_step_poses: the materialised gather, the pose Adam; with a depth prior the depth backward's slots and the
    v_alpha instance of the colour backward.  everything: the six registrations of
    test_all_six_registrations_combine_and_v_alpha_accumulates_onto_the_depth_priors at once."""
    def run(ctx):
        import torch
        from starst3r_amd import ops
        import loss_mask_cases as lmc
        s, d = scene(sc), dscene(sc)
        V, H, W = s["V"], s["H"], s["W"]
        P = {k: v.clone() for k, v in d["P"].items()}
        vm, campos = d["w2c"].clone(), d["campos"].clone()
        grads, loss, vvm = nan(23 * s["N"]), nan(1), nan((V, 4, 4))
        m, v = torch.zeros_like(grads), torch.zeros_like(grads)
        pm, pv = torch.zeros(6 * V, device="cuda:0"), torch.zeros(6 * V, device="cuda:0")
        out = {}
        if prior or everything:
            ops.set_depth_prior(ctx, d["gt"], d["prior"], d["prior_w"], DEPTH_FAC)
        if everything:
            x = on_device(("six", sc), lambda: dict(
                Wt=lmc.weights_for("uniform", V, H, W, 11).astype(F),
                E=(np.tile(np.eye(3, 4), (V, 1, 1)) + 0.1 * np.random.default_rng(77).standard_normal((V, 3, 4))).astype(F),
                b=np.random.default_rng(8).uniform(0, 1, (V, 3)).astype(F),
                M=np.random.default_rng(9).uniform(0, 1, (V, H, W)).astype(F),
                Mw=(2.0 * np.random.default_rng(10).uniform(0, 1, (V, H, W))).astype(F)))
            out["v_exposure"], out["v_Ks"] = nan((V, 3, 4)), nan((V, 4))
            ops.set_exposure(ctx, d["gt"], x["E"], out["v_exposure"])
            ops.set_loss_weight(ctx, d["gt"], x["Wt"])
            ops.set_intrinsics_grad(ctx, d["gt"], out["v_Ks"])
            ops.set_background(ctx, d["gt"], x["b"])
            ops.set_alpha_target(ctx, d["gt"], x["M"], x["Mw"], ALPHA_FAC)
        try:
            ops.train_step_poses(ctx, P, vm, d["Ks"], campos, d["gt"], W, H, 0.2, 0.01, 0.01, grads, m, v, LR, B1, B2, EPS, 1,
                                 loss, pm, pv, 1e-4, 1, None, vvm, want_stats=False)
        finally:
            ops.set_depth_prior(ctx, None, None, None)
            if everything:
                ops.set_exposure(ctx, None, None, None); ops.set_loss_weight(ctx, None, None)
                ops.set_intrinsics_grad(ctx, None, None); ops.set_background(ctx, None, None)
                ops.set_alpha_target(ctx, None, None, None)
        out.update(grads=grads, loss=loss, m=m, v=v, viewmats=vm, campos=campos, pose_m=pm, pose_v=pv, v_viewmats=vvm, **P)
        return out
    return run


def _activated(sc):
    """the same Gaussians handed over as log-scales and logits under st3r_ctx_set_activation"""
    def run(ctx):
        from starst3r_amd import ops
        s, d = scene(sc), dscene(sc)
        raw = on_device(("raw", sc), lambda: dict(P=dict(
            s["P"], scales=np.log(s["P"]["scales"]).astype(F),
            opacities=np.log(s["P"]["opacities"] / (1 - np.minimum(s["P"]["opacities"], 0.999))).astype(F))))["P"]
        grads, loss = nan(23 * s["N"]), nan(1)
        prev = ops.set_activation(ctx, True)
        try:
            ops.train_fwd_bwd(ctx, raw, d["w2c"], d["Ks"], d["campos"], d["gt"], s["W"], s["H"], 0.2, 0.01, 0.01, grads, loss)
        finally:
            ops.set_activation(ctx, prev)
        return dict(grads=grads, loss=loss)
    return run


def _render(sc):
    def run(ctx):
        from starst3r_amd import ops
        s, d = scene(sc), dscene(sc)
        rgb, alpha, st = ops.render(ctx, d["P"], d["w2c"], d["Ks"], d["campos"], s["W"], s["H"])
        return dict(rgb=rgb, alpha=alpha, _n_isects=st["n_isects"])
    return run


def _render_depth(sc):
    """the stage path of Scene.render_3dgs in its depth mode: rasterization, then the depth blend on the same lists"""
    def run(ctx):
        from starst3r_amd import ops
        s, d = scene(sc), dscene(sc)
        P = d["P"]
        rgb, alpha, info = ops.rasterization(ctx, P["means"], P["quats"], P["scales"], P["opacities"], P["shN"], d["w2c"],
                                             d["Ks"], s["W"], s["H"])
        depth = ops.blend_depth_fwd(ctx, info["_splats"], info["isect_offsets"], info["_flatten_ids_dense"], alpha,
                                    info["_last_ids"], s["V"], s["W"], s["H"])
        return dict(rgb=rgb, alpha=alpha, last_ids=info["_last_ids"], depth=depth, flatten_ids=info["_flatten_ids_dense"])
    return run


# ---- stage calls on blend_cases record sets ----
def _blend_inputs(case_name):
    import blend_cases as bc
    case = bc.get(case_name)
    tpg = case.lists()[0]
    rng = np.random.default_rng(3)
    shape = (case.Cn, case.H, case.W)
    return dict(records=case.records, tpg=tpg.astype(np.int32), v_rgb=rng.standard_normal(shape + (3,)).astype(F),
                v_alpha=rng.standard_normal(shape + (1,)).astype(F), v_depth=rng.standard_normal(shape + (1,)).astype(F),
                gt=rng.uniform(0, 1, shape + (3,)).astype(F))


def _stage(case_name, what):
    def run(ctx):
        import blend_cases as bc
        from starst3r_amd import ops
        case = bc.get(case_name)
        d = on_device(("blend", case_name), lambda: _blend_inputs(case_name))
        Cn, W, H = case.Cn, case.W, case.H
        cum, ids, flat = ops.isect(ctx, d["records"], d["tpg"], case.N, Cn, W, H)
        end_bit = 32 + (case.tw * case.th).bit_length() + Cn.bit_length()
        ids_s, flat_s = ops.sort_pairs(ctx, ids, flat, end_bit)
        off = ops.offsets(ctx, ids_s, Cn, W, H)
        rgb, alpha, last = ops.blend_fwd(ctx, d["records"], off, flat_s, Cn, W, H)
        out = dict(cum=cum, flat=flat_s, offsets=off, rgb=rgb, alpha=alpha, last_ids=last)
        if what == "bwd":
            out["v_splats"] = ops.blend_bwd(ctx, d["records"], off, flat_s, alpha, last, d["v_rgb"], d["v_alpha"], cum, Cn, W, H)
        elif what == "bwd_no_alpha":
            out["v_splats"] = ops.blend_bwd(ctx, d["records"], off, flat_s, alpha, last, d["v_rgb"], None, cum, Cn, W, H)
        else:
            out["v_splats"] = ops.blend_depth_bwd(ctx, d["records"], off, flat_s, alpha, last, d["v_depth"], cum, Cn, W, H)
        return out
    return run


def _raster_train(case_name):
    def run(ctx):
        import blend_cases as bc
        from starst3r_amd import ops
        case = bc.get(case_name)
        d = on_device(("blend", case_name), lambda: _blend_inputs(case_name))
        v, loss = nan((case.Cn * case.N, 12)), nan(1)
        st = ops.raster_train(ctx, d["records"], case.N, case.Cn, d["gt"], case.W, case.H, 0.2, v, loss)
        return dict(v_records=v, loss=loss, _n_isects=st["n_isects"])
    return run


def _sort(n, which):
    def run(ctx):
        from starst3r_amd import ops
        d = on_device(("sort", n), lambda: dict(
            k32=np.random.default_rng(n).integers(0, 2 ** 31 - 1, n).astype(np.int32),
            k64=np.random.default_rng(n + 1).integers(0, 2 ** 40, n).astype(np.int64),
            v=np.random.default_rng(n + 2).permutation(n).astype(np.int32)))
        if which == "radix":
            ko, vo = ops.radix_sort_pairs(ctx, d["k32"], d["v"], 0, 32)
        else:
            ko, vo = ops.sort_pairs(ctx, d["k64"], d["v"], 40)
        return dict(keys=ko, vals=vo)
    return run


def _scan(n):
    def run(ctx):
        from starst3r_amd import ops
        d = on_device(("scan", n), lambda: dict(t=np.random.default_rng(n).integers(0, 9, n).astype(np.int32)))
        cum, total = ops.isect_scan(ctx, d["t"])
        return dict(cum=cum, _total=total)
    return run


def _small_adam(which):
    """the per-view Adam steps on their own: in a history they may follow an asynchronous step whose record count is still
    pending, and then run under the device-side guard (st3r_adam_guard)"""
    def run(ctx):
        import torch
        from starst3r_amd import ops
        V, W, H = 3, 96, 64
        sc = scene("regular/a")
        x = on_device(("small_adam",), lambda: dict(
            vm=sc["w2c"], campos=sc["campos"], Ks=sc["Ks"],
            vvm=0.01 * np.random.default_rng(21).standard_normal((V, 4, 4)).astype(F),
            E=(np.tile(np.eye(3, 4), (V, 1, 1)) + 0.1 * np.random.default_rng(22).standard_normal((V, 3, 4))).astype(F),
            vE=np.random.default_rng(23).standard_normal((V, 3, 4)).astype(F),
            vK=np.random.default_rng(24).standard_normal((V, 4)).astype(F)))
        z = lambda n: torch.zeros(n, device="cuda:0")
        if which == "pose":
            vm, campos, m, v = x["vm"].clone(), x["campos"].clone(), z(6 * V), z(6 * V)
            ops.pose_adam_step(ctx, vm, campos, x["vvm"], m, v, 1e-3, B1, B2, EPS, 1)
            return dict(viewmats=vm, campos=campos, m=m, v=v)
        if which == "exposure":
            E, m, v = x["E"].clone(), z(12 * V), z(12 * V)
            ops.exposure_adam_step(ctx, E, x["vE"], m, v, 1e-3, B1, B2, EPS, 1)
            return dict(exposure=E, m=m, v=v)
        Ks, m, v = x["Ks"].clone(), z(4 * V), z(4 * V)
        ops.intrinsics_adam_step(ctx, Ks, x["vK"], m, v, 1e-3, B1, B2, EPS, 1, None, W, H)
        return dict(Ks=Ks, m=m, v=v)
    return run


# ---- the other families: one small case each ----
def _nn(ctx):
    from starst3r_amd import matching
    def build():
        rng = np.random.default_rng(1100)           # test_gpu_nn.py::test_argmax_vs_float64_bruteforce, (100, 1000)
        q = rng.standard_normal((100, 24)).astype(F); d = rng.standard_normal((1000, 24)).astype(F)
        return dict(q=q / np.linalg.norm(q, axis=1, keepdims=True), d=d / np.linalg.norm(d, axis=1, keepdims=True))
    x = on_device(("nn",), build)
    nn, score = matching.nn_dot_argmax(ctx, x["q"], x["d"], want_score=True)
    return dict(nn=nn, score=score)


def _condense(ctx):
    import condense_cases as cc
    from starst3r_amd import ops
    views, H, W = cc.FOCAL_SHAPES[0][:3]
    n, Hc, Wc, S = cc.CANON_SHAPES[0]
    canon, pp, _ = cc.focal_views(views, H, W)
    X, Cf = cc.canon_case(n, Hc, Wc, S)
    x = on_device(("condense",), lambda: dict(canon=np.asarray(canon, F), X=np.asarray(X, F), Cf=np.asarray(Cf, F)))
    c, c2, cconf = ops.canon_view(ctx, x["X"], x["Cf"], S)
    return dict(focals=ops.focal_weiszfeld_batch(ctx, x["canon"], pp), canon=c, canon2=c2, cconf=cconf)


def _dense(ctx):
    import dense_cases as dc
    from starst3r_amd import ops
    c = dc.mixed_case("c3")
    x = on_device(("dense",), lambda: dict(
        start=np.asarray(c["start"], np.int32), pix=np.asarray(c["pix"], F), idx=np.asarray(c["idx"], np.int32),
        off=np.asarray(c["off"], F), core=np.asarray(c["core"], F), cam=np.asarray(c["cam"], F),
        base_f=np.asarray(c["base_f"], F), sizes=np.asarray(c["sizes"], np.int32), conf=np.asarray(c["conf"], F)))
    pts, z = ops.dense_unproject(ctx, x["start"], x["pix"], x["idx"], x["off"], x["core"], x["cam"], x["base_f"])
    conf = ops.dense_clean(ctx, x["start"], x["sizes"], x["cam"], pts, z, x["conf"], tol=0.001, bad_conf=0.0)
    return dict(pts=pts, z=z, conf=conf)


def _align(ctx):
    """one Adam iteration of the alignment on the first single-step case of align_cases (align.run takes the process's own
    context: the runner makes `ctx` that context for the call)"""
    import torch
    import align_cases as ac
    from starst3r_amd import align
    case = ac.get(ac.SINGLE[0])
    res, params = align.run(case.flat, niter1=1, niter2=0, prev_params=case.params, **dict(case.kw))
    out = {k: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)) for k, v in res.items()
           if k in ("intrinsics", "cam2w", "depthmaps", "pts3d", "losses", "_adam_m", "_adam_v")}
    out.update({"p_" + k: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)) for k, v in params.items()})
    return out


def _mcmc(what):
    def run(ctx):
        import torch
        import mcmc_cases as mc
        from starst3r_amd import ops
        N = 257
        if what == "noise":
            P = mc.noise_case(N)
            D = {k: v.clone() for k, v in on_device(("mcmc_noise",), lambda: dict(P=P))["P"].items()}
            ops.mcmc_noise(ctx, D, 500.0, seed=(3 << 32) | 1, step=6)
            return dict(means=D["means"])
        c = mc.exact_case(N)
        D = {k: v.clone() for k, v in on_device(("mcmc",), lambda: dict(P=c["P"]))["P"].items()}
        out = {}
        if what == "relocate":
            n = ops.mcmc_relocate(ctx, D, None, None, c["min_opacity"], seed=c["seed"], step=c["step"])
            st = ops.peek(ctx, 6, 2 * N, torch.int32)
            out.update(_n_dead=n, sampled=st[:n].clone(), dead_ids=st[N:N + n].clone())
        else:
            n_new = c["n_new"]
            D = {k: torch.cat([v, torch.full((n_new,) + tuple(v.shape[1:]), float("nan"), device="cuda:0")]) for k, v in D.items()}
            ops.mcmc_add(ctx, D, N, n_new, c["min_opacity"], seed=c["seed"], step=c["step"])
            out.update(sampled=ops.peek(ctx, 6, n_new, torch.int32))
        out.update(cum=ops.peek(ctx, 4, N, torch.int64), count=ops.peek(ctx, 7, N, torch.int32), **D)
        return out
    return run


BLEND_SETS = ("uneq", "eq257_v2")          # blend_cases: list depths 73 and 257 -- under and over a forward batch of 256
CALLS = {}


def _add(name, run, kind="other", sc=None):
    CALLS[name] = Call(name, run, kind, SCENES[sc][1] if sc else 0, sc)


for _sc in SCENES:
    _add("fwd_bwd:" + _sc, _fwd_bwd(_sc), "train", _sc)
    _add("render:" + _sc, _render(_sc))
for _sc in ("regular/a", "regular/b", "large/a", "large/b", "one_view", "four_views"):
    _add("steps:" + _sc, _steps(_sc), "train", _sc)
for _sc in ("regular/a", "regular/b", "large/a", "large/b"):
    _add("poses:" + _sc, _poses(_sc, False), "train", _sc)
    _add("poses_prior:" + _sc, _poses(_sc, True), "train", _sc)
for _n, _tag in ((1, "step1"), (2, "steps2"), (4, "steps4")):
    _add(_tag + ":regular/a", _steps("regular/a", _n), "train", "regular/a")
for _w in ("pose", "exposure", "intrinsics"):
    _add(_w + "_adam", _small_adam(_w))
_add("fwd_bwd_async:regular/a", _fwd_bwd("regular/a", stats=False), "train", "regular/a")
_add("all_six:regular/a", _poses("regular/a", True, everything=True), "train", "regular/a")
_add("activated:regular/a", _activated("regular/a"), "train", "regular/a")
_add("render_depth:regular/a", _render_depth("regular/a"))
for _c in BLEND_SETS:
    _add("blend_bwd:" + _c, _stage(_c, "bwd"))
    _add("blend_bwd_no_alpha:" + _c, _stage(_c, "bwd_no_alpha"))
    _add("blend_depth_bwd:" + _c, _stage(_c, "depth"))
    _add("raster_train:" + _c, _raster_train(_c))
for _n in (SORT_TILE - 1, SORT_TILE + 1):
    _add("radix_sort:%d" % _n, _sort(_n, "radix"))
    _add("sort_pairs:%d" % _n, _sort(_n, "pairs"))
for _n in (1000, 5000):
    _add("isect_scan:%d" % _n, _scan(_n))
_add("nn", _nn); _add("condense", _condense); _add("dense", _dense); _add("align", _align)
for _w in ("relocate", "add", "noise"):
    _add("mcmc_" + _w, _mcmc(_w))

# the calls that may stand in a seeded shuffle (everything; `align` once per draw is as cheap as the others)
SHUFFLE = sorted(CALLS)
