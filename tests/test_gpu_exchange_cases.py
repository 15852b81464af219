"""GPU parity of the gradient exchange (csrc/comm.hip) and of the range, piece and stage paths of csrc/adam.hip on every
piece, tail, range and block edge of tests/exchange_cases.py (CPU pins: test_oracle_exchange_cases.py).

  1  pieces and stages in one process: w virtual ranks by hand (st3r_adam_step_range, st3r_params_from_stage) against the
     C oracle's Adam on the whole buffer, test_gpu_adam.check's bounds, two steps;
  2  range edges under a one-rank communicator: st3r_gs_train_step with ranges / rs_ag / direct at N = 4095 .. 4099
     against the two-call path, bit for bit;
  3  worlds 2, 3 and 4 (emulated ranks on one GPU through test_gpu_multi's machinery, real ranks where the GPUs are there):
     every form against the float32 sum of the ranks' own gradient buffers in rank order -- the first moment and the
     gradient buffer to the bit, parameters and v against the oracle's Adam on that sum.

The workers of part 3 never assert (a rank that stops between two collectives strands its peers): they save what they
have, the parent judges."""
import os
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import exchange_cases as xc
import loss_adam_cases as lac
import test_gpu_multi as mg
from test_gpu_adam import check, offset_buffer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -12345.0
# Deadline of one world's workers.  Measured on one MI355X: the workers of worlds 2 / 3 / 4 are back after 2.7 / 3.4 /
# 3.5 s; a world that is not back after ten times that, with room for a loaded machine, has lost a
# rank.  The stand-in's own barrier would give up after 120 s.
WORLD_DEADLINE_S = 60.0


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. pieces and stages in one process
@pytest.fixture(scope="module")
def ctx():
    from starst3r_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = ops.Context(DEV)           # private: no state of earlier tests, no communicator
    yield c
    c.close()


def run_pieces(ctx, N, w, misalign_stage=False, compact_sh=False):
    """Two steps of the rs_ag form with the collectives done by hand.  Returns the per-step worst error over bound."""
    from starst3r_amd import ops
    R = xc.piece_reference(N, w, 2, compact_sh)
    total, q, tail0 = xc.layout(N, w)
    ranks = []
    for r in range(w):
        m0, v0, keep = xc.foreign_moments(N, w, r, R["seed"])
        ranks.append(dict(P={k: dev(a) for k, a in R["g0"].items()}, m=dev(m0), v=dev(v0), m0=m0, v0=v0, keep=keep))
    worst = np.zeros(3)
    for step, (gr, P_o, m_o, v_o) in enumerate(R["steps"], 1):
        grads = dev(gr)
        gathered = torch.full((total,), NAN, device=DEV)
        for r, Rk in enumerate(ranks):
            fill = np.full(total, SENTINEL, np.float32)
            stage = offset_buffer(fill) if misalign_stage else dev(fill)
            ops.adam_step_range(ctx, Rk["P"], grads, Rk["m"], Rk["v"], *lac.ADAM_HP, step, r * q, (r + 1) * q, stage)
            ops.adam_step_range(ctx, Rk["P"], grads, Rk["m"], Rk["v"], *lac.ADAM_HP, step, tail0, total)
            st = stage.cpu().numpy()
            outside = np.ones(total, bool); outside[r * q:(r + 1) * q] = False
            assert (st[outside] == SENTINEL).all(), (N, w, r, "the stage outside the piece was written")
            gathered[r * q:(r + 1) * q] = stage[r * q:(r + 1) * q]       # the all-gather
        for r, Rk in enumerate(ranks):
            s = gathered.clone()
            s[r * q:(r + 1) * q] = NAN          # the rank's own piece and the tail of the stage must not be read
            s[tail0:] = NAN
            ops.params_from_stage(ctx, Rk["P"], s, r * q, (r + 1) * q, tail0)
        torch.cuda.synchronize()
        first = None
        for r, Rk in enumerate(ranks):
            P = {k: t.cpu().numpy() for k, t in Rk["P"].items()}
            m, v = Rk["m"].cpu().numpy(), Rk["v"].cpu().numpy()
            own = ~Rk["keep"]
            assert all(np.isfinite(a).all() for a in P.values()), (N, w, r, step)
            check(f"pieces N={N} w={w} rank {r} step {step}", (P, m[own], v[own]), (P_o, m_o[own], v_o[own]), R["g0"])
            # what the rank does not own keeps the bits it started with
            assert np.array_equal(bits(m)[Rk["keep"]], bits(Rk["m0"])[Rk["keep"]]), (N, w, r, step)
            assert np.array_equal(bits(v)[Rk["keep"]], bits(Rk["v0"])[Rk["keep"]]), (N, w, r, step)
            if first is None:
                first = P
            for k in P:
                assert np.array_equal(bits(P[k]), bits(first[k])), (N, w, r, step, k)
            worst = np.maximum(worst, xc.over_bounds(xc.pack(P), m[own], v[own], xc.pack(P_o), m_o[own], v_o[own]))
    print(f"EXCHANGE pieces N={N} w={w}: worst error over bound, parameters {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    return ranks


@pytest.mark.parametrize("N,w", xc.PIECE_CASES)
def test_pieces_reassemble_the_oracle_update(ctx, N, w):
    run_pieces(ctx, N, w)


def test_misaligned_stage_takes_the_scalar_kernel(ctx):
    """(336, 4) with the stage 4 bytes off a 16-byte boundary: st3r_adam_impl's aligned16 covers the stage, so every piece
    goes through k_adam (exchange_cases.piece_tags) and meets the same bounds.  Bit-equality with the aligned run is
    printed, not asserted: the two kernels may contract v differently."""
    a = run_pieces(ctx, 336, 4, misalign_stage=True)
    b = run_pieces(ctx, 336, 4)
    eq = {k: all(torch.equal(x["P"][k], y["P"][k]) for x, y in zip(a, b)) for k in lac.ADAM_NAMES}
    eq["m"] = all(torch.equal(x["m"], y["m"]) for x, y in zip(a, b))
    eq["v"] = all(torch.equal(x["v"], y["v"]) for x, y in zip(a, b))
    print(f"EXCHANGE pieces (336, 4): k_adam (stage misaligned) against k_adam4, bit-equal: {eq}")


def test_pieces_on_a_compact_sh_tensor(ctx):
    """ops passes the SH tensor's own row stride (sh_stride_of): [N, 4, 3] is sh_stride 12, still a multiple of four"""
    from starst3r_amd import ops
    assert ops.sh_stride_of(torch.empty(336, 4, 3)) == 12 and ops.sh_stride_of(torch.empty(336, 24, 3)) == 72
    run_pieces(ctx, 336, 4, compact_sh=True)


# ---------------------------------------------------------------------------------------------------------------------
# 2. range edges under a one-rank communicator
@pytest.fixture(scope="module")
def one_rank():
    from starst3r_amd import dist as sdist, ops
    c = ops.Context(DEV)
    sdist.attach_native_comm(c)
    yield c
    ops.set_exchange(c, "allreduce")
    sdist.detach_native_comm(c)
    c.close()


def _scene_tensors(N, world, away, views, device):
    g, w2c, Ks, gt = xc.scene(N, world, away)
    from starst3r_amd import ops
    P = {k: torch.from_numpy(g[k]).to(device) for k in lac.ADAM_NAMES}
    vm = torch.from_numpy(np.ascontiguousarray(w2c[views])).to(device)
    K = torch.from_numpy(np.ascontiguousarray(Ks[views])).to(device)
    gtv = torch.from_numpy(np.ascontiguousarray(gt[views])).to(device)
    return g, P, vm, K, ops.camera_positions(vm), gtv


def pack_t(P):
    return torch.cat([P[k].reshape(-1) for k, _ in lac.ADAM_BLOCKS] + [P["shN"][:, :4].reshape(-1)])


@pytest.mark.parametrize("form", ["ranges", "rs_ag", "direct"])
@pytest.mark.parametrize("N", xc.RANGE_NS)
def test_one_rank_step_equals_the_two_call_path(one_rank, ctx, N, form):
    """Two steps.  Before each, the two-call side (train_fwd_bwd + adam_step on a context without a communicator) takes
    copies of the state the form is about to step from, so both sides always start from the same bits."""
    from starst3r_amd import _lib, ops
    g, P, vm, K, campos, gt = _scene_tensors(N, 1, False, [0], DEV)
    total = 23 * N
    Kr, _ = xc.ranges(N)
    k_two = xc.adam_kernel(N, 0, total)
    k_form = xc.adam_kernel(N, 0, total, by_gaussian=(form == "ranges" and Kr > 1))
    assert (k_two != k_form) == (form == "ranges" and N == 4096)
    ops.set_exchange(one_rank, form)
    m = torch.zeros(total, device=DEV); v = torch.zeros(total, device=DEV)
    for step in (1, 2):
        A = {k: t.clone() for k, t in P.items()}; ma, va = m.clone(), v.clone()
        before = (pack_t(P).cpu().numpy(), m.cpu().numpy(), v.cpu().numpy())
        gb = torch.full((total,), NAN, device=DEV); lb = torch.zeros(1, device=DEV)
        try:
            ops.train_step(one_rank, P, vm, K, campos, gt, xc.VIEW_W, xc.VIEW_H, *xc.TRAIN_HP, gb, m, v, *lac.ADAM_HP, step, lb)
            ops.settle(one_rank)
        except _lib.St3rError as e:
            if form == "direct" and "direct exchange" in str(e):
                pytest.skip(str(e))                       # the form's own refusal (no exportable uncached memory)
            raise
        ga = torch.full((total,), NAN, device=DEV); la = torch.zeros(1, device=DEV)
        ops.train_fwd_bwd(ctx, A, vm, K, campos, gt, xc.VIEW_W, xc.VIEW_H, *xc.TRAIN_HP, ga, la)
        ops.adam_step(ctx, A, ga, ma, va, *lac.ADAM_HP, step)
        torch.cuda.synchronize()
        tag = f"N={N} {form} step {step}"
        assert float(la) == pytest.approx(float(lb), rel=1e-6), tag
        ga_n, gb_n = ga.cpu().numpy(), gb.cpu().numpy()
        assert np.isfinite(ga_n).all() and np.count_nonzero(ga_n) > total // 2, tag
        assert np.array_equal(bits(gb_n), bits(ga_n)), tag          # grads_out's block layout rebuilt from the range-major stage
        assert np.array_equal(bits(m.cpu().numpy()), bits(ma.cpu().numpy())), tag
        pb, pa = pack_t(P).cpu().numpy(), pack_t(A).cpu().numpy()
        assert np.array_equal(bits(P["shN"][:, 4:].cpu().numpy()), bits(g["shN"][:, 4:])), tag
        eq_v = np.array_equal(bits(v.cpu().numpy()), bits(va.cpu().numpy()))
        eq_p = np.array_equal(bits(pb), bits(pa))
        if k_two == k_form:
            assert eq_v and eq_p, (tag, eq_v, eq_p)
        else:
            # k_adam4 against the ranged k_adam: the two may contract v differently -- both are held to the oracle
            print(f"EXCHANGE one rank {tag}: {k_form} against {k_two}, bit-equal: v {eq_v} parameters {eq_p}")
            p_o, m_o, v_o = xc.oracle_step(*before, ga_n, step)
            for side, (p_, m_, v_) in (("form", (pb, m, v)), ("two-call", (pa, ma, va))):
                xc.assert_check_bounds(f"{tag} {side}", p_, m_.cpu().numpy(), v_.cpu().numpy(), p_o, m_o, v_o)


# ---------------------------------------------------------------------------------------------------------------------
# 3. several ranks
def _key(*parts):
    return "__".join(str(p) for p in parts)


def _any_rank_failed(err, device):
    """Host-side agreement (torch.distributed, not the library's communicator): has any rank an error?  Every rank asks at
    the same points, so all of them leave the case loop together and nobody waits in a collective for a rank that left."""
    t = torch.tensor([1.0 if err else 0.0], device="cpu" if mg.EMULATED else device)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    return bool(t.item() > 0)


def _world_worker(rank, world, port, outdir):
    os.environ["ST3R_XBAR_TIMEOUT_MS"] = "5000"       # a lost peer ends as ST3R_ERR_PEER in seconds
    res, err, ctx, device, T = {}, "", None, None, {}
    Wv, Hv = xc.VIEW_W, xc.VIEW_H

    def save():                                        # (again after the tear-down: whatever a rank has is on disk early)
        res["error"] = np.array(err)
        tmp = os.path.join(outdir, f"rank{rank}.tmp.npz")
        np.savez(tmp, **res)
        os.replace(tmp, os.path.join(outdir, f"rank{rank}.npz"))

    try:
        mg._init(rank, world, port)
    except Exception:                                  # no process group: nothing to agree over, nothing attached
        err = traceback.format_exc()
        save()
        return
    try:
        from starst3r_amd import dist as sdist, ops
        device = mg._device(rank)
        ctx = ops.get_context(device)
        for name, N, away in xc.WORLD_CASES:          # the rank's own gradient buffer, no communicator attached
            g, P0, vm, K, campos, gt = _scene_tensors(N, world, away, [rank], device)
            T[name] = (g, P0, vm, K, campos, gt)
            gr = torch.full((23 * N,), NAN, device=device); loss = torch.zeros(1, device=device)
            ops.train_fwd_bwd(ctx, {k: t.clone() for k, t in P0.items()}, vm, K, campos, gt, Wv, Hv, *xc.TRAIN_HP, gr, loss)
            torch.cuda.synchronize()
            res[_key(name, "g1")] = gr.cpu().numpy(); res[_key(name, "loss")] = loss.cpu().numpy()
    except Exception:
        err = traceback.format_exc()
    attached = False
    if not _any_rank_failed(err, device):
        try:
            sdist.attach_native_comm(ctx)
            attached = True
        except Exception:
            err = traceback.format_exc()
    stop = _any_rank_failed(err, device)
    for name, N, away in xc.WORLD_CASES:
        for form in xc.FORMS:
            for step in (1, 2):
                if stop:
                    break
                try:
                    if step == 1:
                        g, P0, vm, K, campos, gt = T[name]
                        ops.set_exchange(ctx, form)
                        P = {k: t.clone() for k, t in P0.items()}
                        gr = torch.zeros(23 * N, device=device); m = torch.zeros_like(gr); v = torch.zeros_like(gr)
                        loss = torch.zeros(1, device=device)
                    else:                              # the rank's own gradient at the parameters step 1 left, on a copy
                        g2 = torch.full((23 * N,), NAN, device=device); l2 = torch.zeros(1, device=device)
                        ops.train_fwd_bwd(ctx, {k: t.clone() for k, t in P.items()}, vm, K, campos, gt, Wv, Hv,
                                          *xc.TRAIN_HP, g2, l2)
                        torch.cuda.synchronize()
                        res[_key(name, form, "g2")] = g2.cpu().numpy()
                    ops.train_step(ctx, P, vm, K, campos, gt, Wv, Hv, *xc.TRAIN_HP, gr, m, v, *lac.ADAM_HP, step, loss)
                    ops.settle(ctx)
                    torch.cuda.synchronize()
                    for what, t in (("p", pack_t(P)), ("grads", gr), ("m", m), ("v", v), ("loss", loss)):
                        res[_key(name, form, step, what)] = t.cpu().numpy()
                    res[_key(name, form, step, "sh_rest_kept")] = np.array(
                        np.array_equal(bits(P["shN"][:, 4:].cpu().numpy()), bits(g["shN"][:, 4:])))
                except Exception:                      # a library error (or anything else): said, not asserted
                    err = f"{name} {form} step {step}:\n" + traceback.format_exc()
                # a failing rank has still issued every collective of its step (csrc/comm.hip), so its peers arrive here too
                stop = _any_rank_failed(err, device)
    save()
    try:                                               # every rank is here: the tear-down's collectives find their peers
        if attached:
            sdist.detach_native_comm(ctx)
        torch.distributed.destroy_process_group()
    except Exception:
        err += traceback.format_exc()
        save()


class _Worlds:
    """Spawns each world once, on first use; after a world that missed its deadline nothing else is started."""

    def __init__(self, base):
        self.base, self.done, self.lost = base, {}, False

    def get(self, world):
        if world not in self.done:
            self.done[world] = self._run(world)
        W = self.done[world]
        assert W["ok"], W["why"]
        return W

    @staticmethod
    def _said(outdir, world):
        """what the ranks' result files say about a world that did not come back whole"""
        out = []
        for r in range(world):
            f = os.path.join(outdir, f"rank{r}.npz")
            out.append(f"rank {r}: " + ((str(np.load(f)["error"]) or "no error, file written") if os.path.exists(f) else "no file"))
        return " | ".join(out)

    def _run(self, world):
        from starst3r_amd import ops
        if mg.FORCED:
            pytest.skip("ST3R_TEST_MULTI_FORCE=1: one rank on real RCCL only")
        if not mg.EMULATED and world > mg.N_GPUS:
            pytest.skip(f"{world} real ranks need {world} GPUs ({mg.N_GPUS} visible; emulation needs exactly one)")
        if self.lost:
            return dict(ok=False, why="an earlier world missed its deadline: nothing further is started")
        outdir = os.path.join(self.base, f"world{world}")
        os.makedirs(outdir)
        t0 = time.perf_counter()
        pc = mp.spawn(_world_worker, args=(world, mg._free_port(), outdir), nprocs=world, join=False)
        try:
            while not pc.join(timeout=1.0):
                if time.perf_counter() - t0 > WORLD_DEADLINE_S:
                    for p in pc.processes:
                        p.terminate()
                    for p in pc.processes:
                        p.join(10)
                    self.lost = True
                    return dict(ok=False, why=f"world {world}: the ranks were not back after {WORLD_DEADLINE_S:.0f} s; "
                                              + self._said(outdir, world))
        except Exception as e:                          # a rank died: the files say how far the others came
            return dict(ok=False, why=f"world {world}: {e}; " + self._said(outdir, world))
        seconds = time.perf_counter() - t0
        print(f"EXCHANGE world {world} ({'emulated' if mg.EMULATED else 'real'} ranks): workers {seconds:.1f} s")
        # the one-process call over all w views, once per case (the parametrised comparisons touch no GPU)
        ctx = ops.Context(DEV)
        losses = {}
        for name, N, away in xc.WORLD_CASES:
            g, P, vm, K, campos, gt = _scene_tensors(N, world, away, list(range(world)), DEV)
            gr = torch.empty(23 * N, device=DEV); loss = torch.zeros(1, device=DEV)
            ops.train_fwd_bwd(ctx, P, vm, K, campos, gt, xc.VIEW_W, xc.VIEW_H, *xc.TRAIN_HP, gr, loss)
            torch.cuda.synchronize()
            losses[name] = float(loss)
        ctx.close()
        files = [os.path.join(outdir, f"rank{r}.npz") for r in range(world)]
        missing = [f for f in files if not os.path.exists(f)]
        if missing:
            return dict(ok=False, why=f"world {world}: no result file from {missing}")
        return dict(ok=True, ranks=[np.load(f) for f in files], losses=losses, seconds=seconds, real=not mg.EMULATED)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    return _Worlds(str(tmp_path_factory.mktemp("exchange")))


def _region(form, N, world, rank):
    return xc.owned(N, world, rank) if form in xc.PIECEWISE else np.ones(23 * N, bool)


@pytest.mark.parametrize("form", xc.FORMS)
@pytest.mark.parametrize("case", xc.WORLD_CASES, ids=[c[0] for c in xc.WORLD_CASES])
@pytest.mark.parametrize("world", xc.WORLDS)
def test_every_form_delivers_the_rank_ordered_sum(worlds, world, case, form):
    Wd = worlds.get(world)
    name, N, away = case
    Z = Wd["ranks"]
    for r in range(world):
        assert str(Z[r]["error"]) == "", (r, str(Z[r]["error"]))
    total, q, tail0 = xc.layout(N, world)
    # the stand-in adds in rank order, k_xreduce adds in rank order, two ranks commute; RCCL's order past two is its own
    exact = (not Wd["real"]) or world == 2 or form == "direct"
    g0 = xc.scene(N, world, away)[0]
    state = (xc.pack(g0), np.zeros(total, np.float32), np.zeros(total, np.float32))
    for step in (1, 2):
        gs = [Z[r][_key(name, "g1") if step == 1 else _key(name, form, "g2")] for r in range(world)]
        assert all(np.isfinite(x).all() for x in gs), (name, form, step)
        S = xc.rank_ordered_sum(gs)
        slack = (world - 1) * 2.0 ** -24 * np.sum([np.abs(x.astype(np.float64)) for x in gs], axis=0)
        if away and step == 1:                          # the last rank sees nothing: the two regularisers alone
            sl = lac.adam_block_slices(N)
            lone = gs[-1].copy(); lone[sl["scales"]] = 0; lone[sl["opacities"]] = 0
            assert not lone.any() and gs[-1][sl["opacities"]].all() and gs[-1][sl["scales"]].all()
        assert np.count_nonzero(S) >= 11, (name, form, step)
        got = [{k: Z[r][_key(name, form, step, k)] for k in ("p", "grads", "m", "v", "loss")} for r in range(world)]
        for r in range(world):
            reg = _region(form, N, world, r)
            G = got[r]
            assert bool(Z[r][_key(name, form, step, "sh_rest_kept")]), (r, step)
            if exact:
                assert np.array_equal(bits(G["grads"])[reg], bits(S)[reg]), (r, step, "grads are not the rank-ordered sum")
            else:
                assert (np.abs(G["grads"].astype(np.float64) - S)[reg] <= slack[reg]).all(), (r, step)
            if step == 1:                               # from zero moments m decodes the exchanged gradient exactly
                want = xc.first_moment_bits(S if exact else G["grads"])
                assert np.array_equal(bits(G["m"])[reg], want[reg]), (r, "m is not round32(float32(0.1) * S)")
                assert not bits(G["m"])[~reg].any() and not bits(G["v"])[~reg].any(), (r, "moments outside piece and tail")
            assert np.array_equal(bits(G["p"]), bits(got[0]["p"])), (r, step, "replicas differ")
        # rank 0 against the oracle's Adam on S, from the state the step started from
        p_o, m_o, v_o = xc.oracle_step(*state, S, step)
        reg = _region(form, N, world, 0)
        sel = np.ones(total, bool) if exact else np.abs(S) > 1000 * slack
        G = got[0]
        e = xc.over_bounds(G["p"][sel], G["m"][reg & sel], G["v"][reg & sel], p_o[sel], m_o[reg & sel], v_o[reg & sel])
        print(f"EXCHANGE world {world} {name} {form} step {step}: error over bound, parameters {e[0]:.3f} m {e[1]:.3f} v {e[2]:.3f}")
        xc.assert_check_bounds(f"world {world} {name} {form} step {step}", G["p"][sel], G["m"][reg & sel], G["v"][reg & sel],
                               p_o[sel], m_o[reg & sel], v_o[reg & sel])
        # the next step starts from what the ranks hold: under the piece-wise forms the moments live with their owners
        m1, v1 = G["m"].copy(), G["v"].copy()
        if form in xc.PIECEWISE:
            for r in range(1, world):
                m1[r * q:(r + 1) * q] = got[r]["m"][r * q:(r + 1) * q]
                v1[r * q:(r + 1) * q] = got[r]["v"][r * q:(r + 1) * q]
        state = (G["p"], m1, v1)
        if step == 1:                                   # the summed loss: the one-process call over all w views
            for which in (sum(float(Z[r][_key(name, "loss")][0]) for r in range(world)),
                          sum(float(got[r]["loss"][0]) for r in range(world))):
                assert which == pytest.approx(Wd["losses"][name], rel=1e-5), (name, form)
