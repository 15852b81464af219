"""The call sequence of gs.run_3dgs_optim, recorded on the CPU: `gs.ops` is replaced by a stand-in that logs every call,
so a trace says which library calls a training call makes, in which order, with which scalars and which buffers.  Shared
by tests/test_host_train_loop.py and tools/gen_train_loop_trace.py (which writes tests/golden/train_loop_trace.json); only
`gs.ops` is patched and only public results are read, so the same code records any version of gs.py.  No GPU needed."""
import itertools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_loop_trace.json")
ITERS = 3
STEP_CALLS = ("train_step_poses", "train_step", "train_fwd_bwd")
OPTIONS = ("poses", "depth", "exposure", "intrinsics")


class _Ctx:
    native_comm = False


class RecordingOps:
    """Stands where gs.py imports `ops`: every attribute is a function that appends (name, args, kwargs) to `log` and
    returns None, except get_context (a dummy ctx), gt_moments (zeros) and camera_positions (the real one, not logged).
    fail: {"step": {k: code}, "settle": code} -- the k-th step call (1-based, over STEP_CALLS) / settle raises
    _lib.St3rError with that code, after it was logged."""

    def __init__(self, fail=None):
        self.log, self.fail, self.n_steps = [], dict(fail or {}), 0
        self._ctx, self._labels, self._seen = _Ctx(), {}, []

    def _rec(self, x):
        if torch.is_tensor(x):
            self._seen.append(x)   # kept alive: no storage address is used twice
            label = self._labels.setdefault(x.untyped_storage().data_ptr(), len(self._labels))
            return ["tensor", label, x.storage_offset(), list(x.shape), str(x.dtype)]
        if isinstance(x, dict):
            return {str(k): self._rec(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [self._rec(v) for v in x]
        if x is self._ctx:
            return "ctx"
        if x is None or isinstance(x, (bool, int, float, str)):
            return x
        return str(x)   # (a torch.device)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.log.append([name, self._rec(args), self._rec(kwargs)])
            code = None
            if name in STEP_CALLS:
                self.n_steps += 1
                code = self.fail.get("step", {}).get(self.n_steps)
            elif name == "settle":
                code = self.fail.get("settle")
            if code is not None:
                from starst3r_amd import _lib
                err = _lib.St3rError(f"st3r error {code}: injected")
                err.code = code
                raise err
            if name == "get_context":
                return self._ctx
            if name == "gt_moments":
                return torch.zeros(tuple(args[1].shape) + (2,))
            return None
        return call

    @staticmethod
    def camera_positions(viewmats):
        from starst3r_amd import ops
        return ops.camera_positions(viewmats)


def cpu_scene(V=3, N=50, W=32, H=24):
    """_cpu_scene of tests/test_host_intrinsics.py, with depth maps, confidences above the default depth_conf_thres,
    and the strategy / optimizers init_3dgs sets"""
    import starst3r_amd as st
    from starst3r_amd import gs
    from st3r_synth import synth
    g, w2c, Ks = synth.make_scene(N, V, W, H, seed=3)
    scene = st.Scene(device="cpu")
    scene.imgs = [np.zeros((H, W, 3), np.float32) for _ in range(V)]
    scene.c2w = torch.inverse(torch.tensor(w2c).double()).float()
    scene.intrinsics = torch.tensor(Ks)
    scene.gaussians = {k: torch.nn.Parameter(torch.tensor(v)) for k, v in g.items()}
    scene._gs_optim = gs._OptimState(scene, 1e-3)
    scene.optimizers = {k: gs.FusedAdam(scene._gs_optim, k) for k in scene.gaussians}
    scene.strategy = gs.MCMCStrategy()
    scene.strategy_state = scene.strategy.initialize_state()
    scene.depth_maps = [np.full((H, W), 2.0, np.float32) for _ in range(V)]
    scene.depth_confs = [np.full((H, W), 2.0, np.float32) for _ in range(V)]
    return scene


def _pose_rate(step):
    return 1e-4 * (step + 1)


def _k_rate(step):
    return 1e-3 * (step + 2)


def _cases():
    """name -> (options on, fail, enable_pruning)"""
    cases = {}
    for bits in itertools.product((False, True), repeat=4):
        on = tuple(o for o, b in zip(OPTIONS, bits) if b)
        cases["+".join(on) or "off"] = (on, None, False)
    cases["all_capacity_at_step_call_2"] = (OPTIONS, {"step": {2: -3}}, False)
    cases["all_capacity_at_step_call_1"] = (OPTIONS, {"step": {1: -3}}, False)
    cases["all_capacity_at_settle"] = (OPTIONS, {"settle": -3}, False)
    cases["all_peer_error_at_step_call_2"] = (OPTIONS, {"step": {2: -4}}, False)
    cases["off_pruning"] = ((), None, True)
    return cases


CASES = _cases()


def run_case(name):
    """the trace of case `name` as JSON-shaped data: {"log": [[name, args, kwargs], ...], "after": {...}}"""
    from starst3r_amd import _lib, gs
    on, fail, pruning = CASES[name]
    scene = cpu_scene()
    kw = {}
    if "poses" in on:
        kw.update(pose_lr=_pose_rate, pose_freeze=(0,))
    if "depth" in on:
        kw.update(depth_fac=0.1)
    if "exposure" in on:
        kw.update(exposure_lr=2e-3, exposure_freeze=(-1,))
    if "intrinsics" in on:
        scene.intrinsics_lr, scene.intrinsics_freeze = _k_rate, (1,)
    c2w, K = scene.c2w, scene.intrinsics
    rec, real, ret, raised = RecordingOps(fail), gs.ops, None, None
    gs.ops = rec
    try:
        ret = gs.run_3dgs_optim(scene, ITERS, pruning, **kw)
    except _lib.St3rError as e:
        raised = f"St3rError {e.code}"
    finally:
        gs.ops = real
    st = scene._gs_optim
    after = {"n_losses": None if ret is None else len(ret), "raised": raised, "step": st.step,
             "c2w_replaced": scene.c2w is not c2w, "intrinsics_replaced": scene.intrinsics is not K,
             "has_exposures": getattr(scene, "exposures", None) is not None}
    after.update({k: getattr(st, k) for k in ("pose_step", "exp_step", "k_step") if hasattr(st, k)})
    return json.loads(json.dumps({"log": rec.log, "after": after}))


def dump(traces):
    """the text of the golden file: one line per logged call"""
    js = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    cases = []
    for name in sorted(traces):
        t = traces[name]
        cases.append(f'{js(name)}:{{"after":{js(t["after"])},"log":[\n' + ",\n".join(js(e) for e in t["log"]) + "\n]}")
    return "{\n" + ",\n".join(cases) + "\n}\n"
