"""bench.py --dump-outputs: what the last timed step handed back is written as float32 .npy files (a fixed, seeded sample
of the Gaussians, the sample's indices in float64), under 64 MB, the same sample for the same arguments.  CPU tensors
stand in for the device ones: the helper only indexes, copies and saves."""
import os

import numpy as np
import torch

import bench
from starst3r_amd import ops


def _state(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g), "quats": torch.randn(N, 4, generator=g),
         "scales": torch.randn(N, 3, generator=g), "opacities": torch.randn(N, generator=g),
         "sh0": torch.randn(N, 1, 3, generator=g), "shN": torch.randn(N, 4, 3, generator=g)}
    bufs = {k: torch.randn(23 * N, generator=g) for k in ("grad", "adam_m", "adam_v")}
    return P, bufs, torch.tensor([0.25])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_a_seeded_sample_of_the_step_outputs(tmp_path):
    N = 300_000                                                  # more than the sample: the sample is taken
    P, bufs, loss = _state(N)
    total = bench.dump_outputs(str(tmp_path / "a"), ops, P, bufs, loss)
    assert total <= 64 << 20
    a = _load(tmp_path / "a")
    idx = a.pop("sample_index")
    assert idx.dtype == np.float64 and idx.size == bench.DUMP_MAX_GAUSSIANS
    idx = idx.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < N
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) + idx.size * 8 == total
    np.testing.assert_array_equal(a["loss"], [0.25])
    for k in P:
        np.testing.assert_array_equal(a[f"param_{k}"], P[k].numpy()[idx])
    for pre, buf in bufs.items():
        for k, t in ops.split_grads(buf, N).items():
            np.testing.assert_array_equal(a[f"{pre}_{k}"], t.numpy()[idx])
    # same arguments -> same sample
    bench.dump_outputs(str(tmp_path / "b"), ops, P, bufs, loss)
    b = _load(tmp_path / "b")
    np.testing.assert_array_equal(b.pop("sample_index").astype(np.int64), idx)
    assert sorted(b) == sorted(a)
    for k in a:
        np.testing.assert_array_equal(b[k], a[k])


def test_small_scene_is_dumped_whole(tmp_path):
    N = 1000
    P, bufs, loss = _state(N, seed=1)
    bench.dump_outputs(str(tmp_path), ops, P, {}, loss)            # (the Gaussian-sharded layout: parameters only)
    a = _load(tmp_path)
    np.testing.assert_array_equal(a["sample_index"], np.arange(N, dtype=np.float64))
    np.testing.assert_array_equal(a["param_means"], P["means"].numpy())
    assert not any(k.startswith("grad_") for k in a)
