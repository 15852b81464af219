"""gs.run_3dgs_optim's call sequence, pinned: which library calls a training call makes, in which order, with which scalars
and which buffers, for every on/off combination of the per-view options, on the capacity-retry paths, when an error
propagates and with enable_pruning -- against tests/golden/train_loop_trace.json (tools/gen_train_loop_trace.py).  What a
registration registers is cleared, and a counter that is rewound is advanced again, on every one of these paths.
No GPU needed."""
import json

import pytest

import train_loop_cases as tlc


@pytest.fixture(scope="module")
def golden():
    with open(tlc.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(tlc.CASES) and len(tlc.CASES) == 21


@pytest.mark.parametrize("name", list(tlc.CASES))
def test_run_3dgs_optim_makes_the_recorded_calls(golden, name):
    got, want = tlc.run_case(name), golden[name]
    assert got["after"] == want["after"]
    for i, (g, w) in enumerate(zip(got["log"], want["log"])):
        assert g == w, f"call {i} differs"
    assert len(got["log"]) == len(want["log"])


def test_the_traces_have_the_expected_sizes(golden):
    """an all-off call logs 8 entries, an all-on call 20 (and the recorder is not vacuous)"""
    assert len(golden["off"]["log"]) == 8 and len(golden["+".join(tlc.OPTIONS)]["log"]) == 20
    names = [e[0] for e in golden["+".join(tlc.OPTIONS)]["log"]]
    assert names[2:6] == ["set_gt_moments", "set_depth_prior", "set_exposure", "set_intrinsics_grad"] == names[-4:]
