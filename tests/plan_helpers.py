"""What the two launch-plan tiers (tests/test_gpu_feature_plans.py: the five full-march kinds of frame; tests/test_gpu_composite_plans.py:
composite frames) share, stated once: the 14 fields of last_launch(), the tiny ragged volume, the hand-built views along a volume axis, the
frame parameters, the comparison against a fixture under tests/golden/, and the printing of such a fixture from two runs
(scripts/feature_launch_plans.py).  What is enumerated, and what one plan holds, stay with each file (its record())."""
import importlib
import json
import sys

import numpy as np

FIELDS = ("layout", "brick_plane", "lane_map", "phase_x", "phase_y", "clamp_fetch", "tiles_x", "tiles_y", "ordered", "straddle_permille", "column_voxels",
          "column_shade_pairs", "shadowed", "run_flavour")
SHAPE = (16, 20, 24)                             # z, y, x: ragged, no edge a multiple of the brick edge but z
VOXELS = ("u8", "u16")
LIGHT = (0.5, -1.0, 3.0)


def volume(voxels):
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, SHAPE)
    return raw.astype(np.uint8) if voxels == "u8" else (raw * 257).astype(np.uint16)


def axis_view(vr, window, axis, perspective, pitch=None):
    """the view along volume axis `axis` (0 x, 1 y, 2 z), built by hand: exact zeros; pitch = model units per pixel (None: 0.045, in
    perspective 0.0125 per pixel and unit of k)"""
    v = vr.VrView()
    v.width, v.height, v.perspective = window[0], window[1], perspective
    for j in range(3):
        v.origin[j] = v.direction[j] = v.right_plane[j] = v.up_plane[j] = 0.0
        v.light_pos[j] = LIGHT[j]
    v.direction[axis], v.origin[axis] = 1.0, -3.0 if perspective else -2.0
    v.right_plane[(axis + 1) % 3] = v.up_plane[(axis + 2) % 3] = pitch if pitch is not None else 0.0125 if perspective else 0.045
    return v


def frame_params(vr, view, sampling, esl, threshold=0.95, light_kd=0.7):
    p = vr.VrParams()
    p.view = view
    p.ray_step, p.ray_threshold, p.light_kd = 0.05, threshold, light_kd
    p.esl, p.esl_block_dims, p.sampling = esl, 3, sampling
    for j in range(3):
        p.esl_block_size[j] = (0.25, 0.3, 0.375)[j]
    return vr.whole_frame(p)


def launched(gpu):
    """the FIELDS of last_launch()"""
    info = gpu.last_launch()
    return [info[f] for f in FIELDS]


def assert_same(got, fixture, prefix):
    want = {k: v for k, v in fixture.items() if k.startswith(prefix)}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    wrong = [(k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not wrong, (len(wrong), wrong[:8])


def print_plans(vr, module, check):
    """Prints the fixture of test module `module` — its record(vr, gpu) in a fresh context — one plan per line.  check: the enumeration
    runs twice, in two fresh contexts, and the process exits 1 if the two differ in any field (a plan is host arithmetic)."""
    plans = importlib.import_module(module)

    def once():
        gpu = vr.HipRenderer(0)
        try:
            return plans.record(vr, gpu)
        finally:
            gpu.close()
    first = once()
    if check:
        second = once()
        differing = [k for k in first["plans"] if first["plans"][k] != second["plans"].get(k)]
        if differing or len(first["plans"]) != len(second["plans"]):
            sys.exit(f"two runs differ in {len(differing)} plans: {[(k, first['plans'][k], second['plans'].get(k)) for k in differing[:8]]}")
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in first["plans"].items())
    sys.stdout.write(f'{{"fields": {json.dumps(first["fields"])},\n "plans": {{\n{rows}\n }}}}\n')
