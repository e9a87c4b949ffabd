#!/usr/bin/env python3
"""feature_launch_plans.py [--check] [test module] — prints the JSON of a launch-plan fixture under tests/golden/: what record() of the
test module enumerates, on the library of this tree.  test_gpu_feature_plans (the default) prints feature_launch_plans.json,
test_gpu_composite_plans prints composite_launch_plans.json.  A fixture pins what the host decided BEFORE a change of the launchers: run
this in a checkout of the commit before the change (with the test module and tests/plan_helpers.py copied in), not on the code under test.
--check runs the enumeration twice in two fresh contexts and exits 1 if the two differ in any field (the plan is host arithmetic)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch  # noqa: F401  (loads the process's HIP runtime first)
    from plan_helpers import print_plans
    modules = [a for a in sys.argv[1:] if not a.startswith("--")]
    print_plans(importlib.import_module("volume-rendering_amd"), modules[0] if modules else "test_gpu_feature_plans", "--check" in sys.argv[1:])


if __name__ == "__main__":
    main()
