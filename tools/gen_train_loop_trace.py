#!/usr/bin/env python
"""Generates tests/golden/train_loop_trace.json: the library calls gs.run_3dgs_optim makes on a small CPU scene, per case of
tests/train_loop_cases.py (every on/off combination of the four per-view options, the capacity-retry paths, a propagating
error, enable_pruning), recorded through a stand-in for `gs.ops`.

The file is the record of what the loop did at the commit it was generated at; tests/test_host_train_loop.py holds every
later gs.py to it, entry for entry.  Regenerate it only for a deliberate change of the call sequence -- a refactor must
reproduce it byte for byte.  Run:  python tools/gen_train_loop_trace.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import train_loop_cases as tlc   # noqa: E402


def main():
    traces = {name: tlc.run_case(name) for name in tlc.CASES}
    with open(tlc.GOLDEN, "w") as f:
        f.write(tlc.dump(traces))
    for name, t in traces.items():
        print(f"{name}: {len(t['log'])} calls, after = {t['after']}")
    print(f"wrote {tlc.GOLDEN} ({os.path.getsize(tlc.GOLDEN) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
