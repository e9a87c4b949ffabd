#!/usr/bin/env python3
"""feature_launch_plans.py [--check] — prints the JSON of tests/golden/feature_launch_plans.json: what vr_hip_last_launch reports for every frame
tests/test_gpu_feature_plans.py enumerates (record() there), on the library of this tree.  The fixture pins what the host decided BEFORE a
change of the launchers: run it in a checkout of the commit before the change (with that test module copied in), not on the code under
test.  --check runs the enumeration twice in two fresh contexts and exits 1 if the two differ in any field (the plan is host arithmetic)."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def once(vr, plans):
    gpu = vr.HipRenderer(0)
    try:
        return plans.record(vr, gpu)
    finally:
        gpu.close()


def main():
    import torch  # noqa: F401  (loads the process's HIP runtime first)
    vr = importlib.import_module("volume-rendering_amd")
    plans = importlib.import_module("test_gpu_feature_plans")
    first = once(vr, plans)
    if "--check" in sys.argv[1:]:
        second = once(vr, plans)
        differing = [k for k in first["plans"] if first["plans"][k] != second["plans"].get(k)]
        if differing or len(first["plans"]) != len(second["plans"]):
            sys.exit(f"two runs differ in {len(differing)} plans: {differing[:8]}")
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in first["plans"].items())      # one plan per line
    sys.stdout.write(f'{{"fields": {json.dumps(first["fields"])},\n "plans": {{\n{rows}\n }}}}\n')


if __name__ == "__main__":
    main()
