"""Context history: every call must give a fresh context's bits.

ops.get_context hands out ONE st3r_ctx per process and GPU, and everything -- matching, condensation, alignment, dense
extraction, the 3DGS steps, the MCMC hooks, the renders -- runs on its grow-only arena for hours.  The context carries
state from call to call that is never cleared per call (csrc/common.h: struct st3r_ctx; the table is in DESIGN.md,
"Context history"): stamped gradient slots and touch stamps, the scans' generation-stamped control blocks, the sort's ticket
counters, the record-count hint, cached weight norms, the sticky chunk count, slot layouts that follow the debug flags.

The property: the outputs of a call are a function of its arguments, the registrations, the debug flags and the chunk count
-- never of what the context ran before.  A history (a list of call names of history_cases.py and context actions) runs on
ONE context; after every call EVERY output is compared, bit for bit, with the same call on a context created for it
alone (same debug flags, same chunk count; cached per call; closed after its call).  That reference is another object than
the path under test -- fresh arena, stamps at 1, no hint -- and the parity suites hold it to the oracles.  The loss
scalars are compared for the same bits like everything else; no history needed the per-view double sums instead.

Every output buffer is poisoned before its call: the catalogue fills the buffers it hands over with NaN, and every call --
in a history and on its fresh context alike -- runs under `poisoned_allocations`, which makes torch.empty / torch.empty_like
(what `ops`, `matching` and `align` allocate their outputs with) return NaN-filled floats and 0x5A-filled integers.  Without
that the caching allocator hands a repeated call the block that still holds its own earlier, correct result, and a call
that wrote nothing would pass.  Measured run time: at the end of this file.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import history_cases as hc

WRAP = 2147483000          # blend_common.h: stamped_slots restarts a counter that has reached this
TRAIN_FLAGS = 32           # the one flag that changes a training call's bits (two view chunks: another association)


def bits(t):
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def first_difference(a, b):
    """None if the two outputs are the same bits (tensors) / equal (host scalars), else a description"""
    if not torch.is_tensor(a):
        return None if a == b else "%r != %r" % (a, b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s != %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    ne = bits(a) != bits(b)
    if not bool(ne.any()):
        return None
    i = int(torch.nonzero(ne)[0])
    return "first differing element %d of %d (%d differ): %r, fresh context %r" % (
        i, ne.numel(), int(ne.sum()), a.reshape(-1)[i].item(), b.reshape(-1)[i].item())


@contextlib.contextmanager
def as_process_context(ctx):
    """align.run and the matching front end take ops.get_context(device): make `ctx` that context for one call"""
    from starst3r_amd import ops
    idx = ctx.device.index
    old = ops._contexts.get(idx)
    ops._contexts[idx] = ctx
    try:
        yield
    finally:
        if old is None:
            del ops._contexts[idx]
        else:
            ops._contexts[idx] = old


@contextlib.contextmanager
def poisoned_allocations():
    """torch.empty and torch.empty_like return poisoned memory (NaN / 0x5A5A...; bool: True) while this is active"""
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.bool:
            t.fill_(True)
        elif t.numel():
            t.view(torch.uint8).fill_(0x5A)
        return t

    torch.empty = lambda *a, **k: poison(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: poison(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def run_call(ctx, call):
    with as_process_context(ctx), poisoned_allocations():
        out = call.run(ctx)
    torch.cuda.synchronize()
    return out


_fresh = {}


def fresh(name, flags=0, chunked=False):
    """the outputs of call `name` on a context created for it alone, under `flags` (and two view chunks if `chunked`)"""
    from starst3r_amd import ops
    call = hc.CALLS[name]
    if call.kind != "train":
        chunked = False          # only the training calls read the chunk count
    key = (name, flags, chunked)
    if key not in _fresh:
        ctx = ops.Context("cuda:0")
        try:
            ops.set_debug(ctx, flags | (TRAIN_FLAGS if chunked else 0))
            _fresh[key] = run_call(ctx, call)
            ops.settle(ctx)
        finally:
            ctx.close()
    return _fresh[key]


class History:
    """one context; `play` runs calls and actions and compares each call with its fresh-context reference"""

    def __init__(self, name):
        from starst3r_amd import ops
        self.name, self.ctx = name, ops.Context("cuda:0")
        self.flags, self.chunked, self.done, self.log = 0, False, [], []

    def play(self, steps, ref_flags=None):
        from starst3r_amd import ops
        for step in steps:
            pos = len(self.done)
            self.done.append(step)
            if isinstance(step, tuple):
                what = step[0]
                if what == "flags":
                    self.flags = step[1]
                    ops.set_debug(self.ctx, step[1])
                elif what == "stamps":
                    ops.debug_set_stamps(self.ctx, step[1], step[2])
                elif what == "release":
                    self.ctx.release_scratch()
                    assert self.ctx.arena_bytes() == 0
                elif what == "settle":
                    ops.settle(self.ctx)
                else:
                    raise ValueError(step)
                continue
            call = hc.CALLS[step]
            before = self.ctx.arena_bytes()
            got = run_call(self.ctx, call)
            if call.kind == "train" and call.views > 1 and (self.flags & TRAIN_FLAGS):
                self.chunked = True                      # view_chunks sticks to the context (fused_step.hip)
            want = fresh(step, (self.flags & ~256) if ref_flags is None else ref_flags, self.chunked)
            assert set(got) == set(want)
            for k in sorted(got):
                d = first_difference(got[k], want[k])
                assert d is None, "history %r, position %d, call %r, output %r: %s\n    reproduce with: %r" % (
                    self.name, pos, step, k, d, self.done)
            self.log.append(dict(call=step, before=before, after=self.ctx.arena_bytes(), n_isects=got.get("_n_isects")))
        return self

    def close(self):
        from starst3r_amd import ops
        torch.cuda.synchronize()
        ops.settle(self.ctx)          # no history may end in ST3R_ERR_CAPACITY: this raises if the last step overflowed
        self.ctx.close()


def play(name, steps, **kw):
    h = History(name)
    try:
        h.play(steps, **kw)
    finally:
        h.close()
    return h


def fb(*scenes):
    return ["fwd_bwd:" + s for s in scenes]


def check_touch_sides(h):
    """the code's own condition for the touch array (st3r_blend_bwd_impl: n > 8 N C), from the calls' statistics"""
    seen = set()
    for e in h.log:
        c = hc.CALLS[e["call"]]
        if e["call"].startswith("fwd_bwd:") and e["n_isects"] is not None:
            N, V = hc.SCENES[c.scene][:2]
            assert (e["n_isects"] > 8 * N * V) == hc.TOUCH[c.scene], e
            assert abs(e["n_isects"] - hc.RECORDS[c.scene]) <= 0.01 * hc.RECORDS[c.scene], e    # the oracle's count, to 1 %
            seen.add(hc.TOUCH[c.scene])
    return seen


# ---- 1. slots: growth and reuse ----
def test_slots_growth_and_reuse():
    """the two scene kinds and their two seeds in turn: every call reads slot ranges that the calls before it stamped and it
    does not write (test_oracle_history_cases.py: a quarter / four fifths of its pairs own such a slot)"""
    h = play("slots", fb("regular/a", "large/a", "regular/b", "large/b", "regular/a", "large/a"))
    assert check_touch_sides(h) == {True, False}
    assert h.log[0]["after"] > h.log[0]["before"] and h.log[1]["after"] > h.log[1]["before"]      # growth ...
    for e in h.log[2:]:
        assert e["after"] == e["before"], e                                                         # ... then reuse


def test_slots_shared_with_the_stage_calls():
    """st3r_gs_blend_bwd shares the stamp counter and the slot buffer with the fused path: both kernels instances of the
    stage call (v_alpha given / NULL) between the fused ones, on record sets of two list depths"""
    play("slots+stages", ["fwd_bwd:regular/a", "blend_bwd:uneq", "fwd_bwd:large/a", "blend_bwd_no_alpha:eq257_v2",
                          "fwd_bwd:regular/b", "blend_bwd:eq257_v2", "fwd_bwd:large/b", "blend_bwd_no_alpha:uneq",
                          "fwd_bwd:regular/a", "raster_train:uneq", "fwd_bwd:large/a", "blend_bwd:uneq"])


# ---- 2. slots: the restart at the wrap ----
@pytest.mark.parametrize("kind", ["regular", "large"])
def test_colour_stamps_restart_at_the_wrap(kind):
    """X/a at stamps 1 .. 3, then X/b at 2147482999, 2147483000, 1 (restart: the slots are zeroed), 2 and 3 -- the last one
    over slot ranges that X/a stamped 3 before the restart"""
    a, b = "fwd_bwd:%s/a" % kind, "fwd_bwd:%s/b" % kind
    play("wrap " + kind, [a, a, a, ("stamps", WRAP - 2, -1), b, b, b, b, b])


def test_depth_stamps_restart_at_the_wrap():
    a, b = "blend_depth_bwd:eq257_v2", "blend_depth_bwd:uneq"
    play("wrap depth, stage", [a, a, a, ("stamps", -1, WRAP - 2), b, b, b, b, b])
    a, b = "poses_prior:regular/a", "poses_prior:regular/b"
    play("wrap depth, fused", [a, a, a, ("stamps", -1, WRAP - 2), b, b, b, b, b])


def test_colour_and_depth_restart_in_different_calls():
    a, b = "poses_prior:large/a", "poses_prior:large/b"
    play("wrap both", [a, a, a, ("stamps", WRAP - 2, WRAP - 3), b, b, b, b, b, b])      # colour restarts in the 3rd, depth in the 4th


# ---- 3. stamps that are not ordinary floats ----
def test_stamps_across_infinity_and_the_nan_patterns():
    """The stamp travels as __int_as_float(stamp) in the slot's last float.  From 0x7F800000 on that is +inf, then the
    signalling NaNs (to 0x7FBFFFFF), then the quiet ones: an instruction that canonicalised it on the way would make every
    slot look stale and every gradient zero.  Six backward calls from 0x7F7FFFFE across +inf (both counters take four
    of them), four across the first quiet pattern 0x7FC00000: both scene kinds, the pose step's materialised gather, the depth
    backward fused and stand-alone, over slots that earlier calls stamped with small integers."""
    play("nan stamps", ["poses_prior:regular/a", "poses_prior:large/a",
                        ("stamps", 0x7F7FFFFD, 0x7F7FFFFD),
                        "poses_prior:regular/b", "blend_depth_bwd:uneq", "poses_prior:large/b", "fwd_bwd:large/a",
                        "poses:regular/a", "blend_depth_bwd:eq257_v2",
                        ("stamps", 0x7FBFFFFE, 0x7FBFFFFE),
                        "poses_prior:large/a", "poses_prior:regular/b", "fwd_bwd:large/b", "blend_depth_bwd:uneq",
                        "blend_bwd:uneq", "fwd_bwd:regular/a"])


# ---- 4. touch stamps ----
def test_touch_stamps_across_growth():
    """dense_small (no TOUCH) grows the slots -- the stamps restart -- while the touch array of the large calls exists; the
    large call after it finds that array again"""
    h = play("touch", fb("large/a", "large/b", "dense_small", "large/b", "regular/a", "large/a"))
    assert check_touch_sides(h) == {True, False}
    assert h.log[1]["after"] == h.log[1]["before"]
    assert h.log[2]["after"] > h.log[2]["before"] and h.log[2]["n_isects"] > 1.25 * max(h.log[0]["n_isects"], h.log[1]["n_isects"])
    assert h.log[3]["after"] == h.log[3]["before"] and h.log[5]["after"] == h.log[5]["before"]


# ---- 5. view chunks ----
def test_view_chunks_stick_and_are_clamped():
    """under debug flag 32 a 3-view call (chunks of 1 and 2 views, each a backward call of its own on the same slots with
    another `cum`); then WITHOUT the flag a 1-view call (the count is clamped to C), a 4-view call and three steps: all of
    them equal a fresh context's under the flag -- the count stuck -- and the 4-view bits are not the one-pass bits"""
    a, b = fresh("fwd_bwd:four_views", 0, True), fresh("fwd_bwd:four_views", 0, False)
    assert first_difference(a["grads"], b["grads"]) is not None      # (else the equality below would say nothing)
    h = play("chunks", [("flags", 32), "fwd_bwd:regular/a", ("flags", 0), "fwd_bwd:one_view", "fwd_bwd:four_views",
                        "steps:regular/a", "poses_prior:large/a", "steps:four_views"])
    assert h.chunked


def test_one_view_under_the_flag_makes_no_chunk_count_stick():
    """the count is clamped to C BEFORE it is written back (`if (chunks > C) chunks = C` ... `if (chunks > 1)
    ctx->view_chunks = chunks`): a 1-view call under flag 32 runs in one chunk and leaves the context unchunked, so the
    4-view call after it, without the flag, gives the ONE-PASS bits (which differ from the chunked ones, asserted above
    and here).  Nothing launches on an empty range either way: train_chunks skips an empty chunk."""
    a, b = fresh("fwd_bwd:four_views", 0, True), fresh("fwd_bwd:four_views", 0, False)
    assert first_difference(a["grads"], b["grads"]) is not None
    h = play("clamp", [("flags", 32), "fwd_bwd:one_view", "steps:one_view", ("flags", 0), "fwd_bwd:four_views",
                       "steps:regular/a"])
    assert not h.chunked


# ---- 6. the record-count hint ----
def test_hint_follows_the_shape_of_the_call():
    """three steps reach the asynchronous steady state; a step on another shape (hint_sig) must take the synchronous path;
    back on the first shape the hint is that of the other scene and the first step sizes exactly again"""
    play("hint", ["steps:regular/a", "steps:one_view", "steps:regular/a", "steps:regular/b", "steps:large/a", "steps:regular/a"])


def test_calls_between_asynchronous_steps():
    """a render, a records call and the per-view Adam steps between asynchronous steps: each small Adam step follows a step
    whose record count is still pending, so it runs under the device-side guard; `settle` at the end"""
    play("hint+guard", ["steps:regular/a", "step1:regular/a", "pose_adam", "step1:regular/a", "exposure_adam",
                        "step1:regular/a", "intrinsics_adam", "step1:regular/a", "render:regular/b", "step1:regular/a",
                        "raster_train:uneq", "step1:regular/a", "fwd_bwd_async:regular/a", "pose_adam", ("settle",)])


# ---- 7. scan generations across entry points ----
MIX = ["render:regular/a", "fwd_bwd:large/a", "isect_scan:1000", "raster_train:uneq", "isect_scan:5000", "render:large/b",
       "fwd_bwd:regular/b", "isect_scan:1000", ("flags", 32), "fwd_bwd:four_views", "raster_train:eq257_v2",
       "fwd_bwd:regular/a", "isect_scan:5000", "render:regular/a", "fwd_bwd:large/a", "isect_scan:1000", "render:one_view"]


@pytest.mark.parametrize("wrap", [False, True])
def test_scan_generations_across_entry_points(wrap):
    """render, train, chunked train, records and the stand-alone scan launch 1, 2 and more scans per call: both launch
    parities meet both ticket counters.  wrap: debug flag 256 before the fourth call puts both scans two or three launches
    before the wrap of their 14-bit generations, so both control blocks are cleared inside the mix"""
    steps = list(MIX)
    if wrap:
        steps[3:3] = [("flags", 256), ("flags", 0)]
    play("scans, wrap=%s" % wrap, steps)


# ---- 8. cached norms ----
NORM_VIEWS = 40            # 40 views x 8 / 16 bytes: past the 256 bytes an arena slot starts with -- the norm slot grows


def _norm_inputs():
    def build():
        from st3r_synth import synth
        import loss_mask_cases as lmc
        N, V, W, H = 400, 5, 96, 64
        g, w2c, Ks = synth.make_scene(N, V, W, H, seed=7, scale_lo=0.01, scale_hi=0.08)
        rng = np.random.default_rng(41)
        return dict(P={k: np.ascontiguousarray(g[k], np.float32) for k in ("means", "quats", "scales", "opacities", "shN")},
                    w2c=w2c.astype(np.float32), Ks=Ks.astype(np.float32),
                    campos=np.linalg.inv(w2c.astype(np.float64))[:, :3, 3].astype(np.float32),
                    gt=rng.uniform(0, 1, (NORM_VIEWS, H, W, 3)).astype(np.float32),
                    payload=rng.uniform(0.2, 5.0, (NORM_VIEWS, H, W)).astype(np.float32),
                    A=lmc.weights_for("uniform", NORM_VIEWS, H, W, 11).astype(np.float32),
                    B=(3.0 * lmc.weights_for("uniform", NORM_VIEWS, H, W, 12)).astype(np.float32),
                    w=np.zeros((NORM_VIEWS, H, W), np.float32))
    return hc.on_device(("norms",), build)


def _register(ctx, kind, x, R):
    from starst3r_amd import ops
    gt = None if R == 0 else x["gt"][:R]
    if kind == "depth_prior":
        ops.set_depth_prior(ctx, gt, None if R == 0 else x["payload"][:R], None if R == 0 else x["w"][:R], hc.DEPTH_FAC)
    elif kind == "loss_weight":
        ops.set_loss_weight(ctx, gt, None if R == 0 else x["w"][:R])
    else:
        ops.set_alpha_target(ctx, gt, None if R == 0 else torch.clamp(x["payload"][:R], 0, 1), None if R == 0 else x["w"][:R],
                             hc.ALPHA_FAC)


def _norm_step(ctx, x, C):
    from starst3r_amd import ops
    grads, loss = hc.nan(23 * 400), hc.nan(1)
    ops.train_fwd_bwd(ctx, x["P"], x["w2c"][:C], x["Ks"][:C], x["campos"][:C], x["gt"][:C], 96, 64, 0.2, 0.01, 0.01, grads, loss)
    torch.cuda.synchronize()
    return dict(grads=grads, loss=loss)


# (weights written into the registered buffer, views registered (0: cleared), views of the step, what happens first)
NORM_STEPS = [("A", 3, 3, "set"),           # the first registration
              ("B", 3, 3, "set"),           # the same pointers again, other weights in them
              ("A", 2, 2, "set"),
              ("A", NORM_VIEWS, 5, "set"),  # the norm slot grows
              ("A", 0, 3, "set"),           # cleared
              ("B", 3, 3, "set+release"),   # set again, then release_scratch
              ("B", 3, 3, "release"),       # release_scratch under a registration whose norms ARE computed: the slot is
                                            # gone, `valid` is not ("grown ||" in st3r_registered_weight_norms)
              ("B", 3, 3, "release+other")] # the same with a call on other views first: it takes the freed blocks, so the
                                            # norm slot does not come back as the block that still holds the old norms


@pytest.mark.parametrize("kind", ["depth_prior", "loss_weight", "alpha_target"])
def test_cached_norms_follow_the_registration(kind):
    """n_c / the weight sums of a registration are computed once, by the first step that uses it, into an arena slot.  The
    reference of every step is a fresh context with that registration alone."""
    from starst3r_amd import ops
    x = _norm_inputs()
    want = []
    for variant, R, C, first in NORM_STEPS:
        ctx = ops.Context("cuda:0")
        x["w"].copy_(x[variant])
        _register(ctx, kind, x, R)
        want.append(_norm_step(ctx, x, C))
        _register(ctx, kind, x, 0)
        ctx.close()
    assert first_difference(want[0]["grads"], want[1]["grads"]) is not None      # the weights matter
    assert first_difference(want[0]["loss"], want[4]["loss"]) is not None        # and so does the registration
    ctx = ops.Context("cuda:0")
    try:
        for pos, (variant, R, C, first) in enumerate(NORM_STEPS):
            x["w"].copy_(x[variant])
            if "set" in first:
                _register(ctx, kind, x, R)
            if "other" in first:
                ctx.release_scratch()
                run_call(ctx, hc.CALLS["fwd_bwd:large/a"])
            elif "release" in first:
                ctx.release_scratch()
                assert ctx.arena_bytes() == 0
            got = _norm_step(ctx, x, C)
            for k in got:
                d = first_difference(got[k], want[pos][k])
                assert d is None, "norms of %s, step %d %r, output %r: %s" % (kind, pos, NORM_STEPS[pos], k, d)
    finally:
        _register(ctx, kind, x, 0)
        ctx.close()


# ---- 9. slot layouts under changing flags ----
@pytest.mark.parametrize("sc", ["regular/a", "large/a"])
def test_flags_change_the_layout_of_shared_slots(sc):
    """64: 64-bit rectangles and no `rectbase`; 1024: two arrays instead of the packed word; 16: the plain emission and the
    two-pass tile sort; 128: the quadrant forward.  Every one of them gives the flag-0 bits on a fresh context (the parity
    suites), so on one context, one after another over each other's slots, every result equals the flag-0 fresh bits."""
    steps = []
    for f in (0, 64, 0, 1024, 16, 128, 0):
        steps += [("flags", f), "fwd_bwd:" + sc, "steps:" + sc]
    play("flags " + sc, steps, ref_flags=0)


def test_activation_on_off_on():
    """the activated step reads exp / sigmoid copies in scratch of its own; the plain step between them must not"""
    play("activation", ["activated:regular/a", "fwd_bwd:regular/a", "activated:regular/a", "steps:regular/a",
                        "activated:regular/a", "all_six:regular/a", "activated:regular/a", "render:regular/a"])


# ---- 10. a whole session ----
SESSION = ["nn", "condense", "align", "align", "align", "dense", "steps4:regular/a", "mcmc_relocate", "mcmc_add",
           "steps2:regular/a", "mcmc_noise", "render:regular/a"]


@pytest.mark.parametrize("release_at", [None] + list(range(1, len(SESSION))))
def test_a_whole_session(release_at):
    """the families in the order a reconstruction runs them, the MCMC hooks between the training steps (SLOT_SCAN_TMP and
    SLOT_SMALL are shared: another family uses the scan and sort scratch in between); then the same list with
    release_scratch() before every position in turn, one context per variant"""
    steps = list(SESSION)
    if release_at is not None:
        steps.insert(release_at, ("release",))
    play("session, release at %s" % release_at, steps)


# ---- 11. seeded shuffles: a net under the planted histories ----
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_shuffles(seed):
    """40 draws from the whole catalogue; the view chunks (which stick) start before the last 8.  A failure prints the prefix
    that reproduces it."""
    rng = np.random.default_rng(seed)
    draws = [hc.SHUFFLE[i] for i in rng.integers(0, len(hc.SHUFFLE), 40)]
    play("shuffle %d" % seed, draws[:32] + [("flags", 32)] + draws[32:])


# MEASURED (MI355X): 35 cases, 3.7 s alone with start-up; the slowest case 0.61 s (the first one: library and scene
# set-up), every other below 0.4 s.  The GPU cases do no oracle work (history_cases.RECORDS is pinned by the CPU file).
# All pass on the unchanged kernels: no history found a defect.
# Mutations (each run once on a scratch copy; the table, the equivalence arguments of the two touch clears, and the two
# mutants that were not run): DESIGN.md, "Context history".
