"""What the host decides for a composite frame — launch_frame (vr_hip_api.cpp): vr_hip_render, vr_hip_render_device, the backdrop pass —,
pinned: every field of last_launch() (the 14 FIELDS of the feature-plans tier, run_flavour among them) and the two masks of resident
copies (volume_info().copies, run_aligned_info()["copies"]: which copies the frame caused to be built — the footprint is behaviour) after
every repetition of tiny frames under every setting the decision branches on, held against tests/golden/composite_launch_plans.json.
Every copy of a volume gives the same pixels, so the parity tiers do not see a frame that reads another copy, maps or orders its tiles
differently, or builds a copy it does not need; this file does.

One row is a SEQUENCE of repetitions of one frame on one context, because `ordered`, the measured validator of the per-tile run-copy
choice (vr_hip_set_brick_plane(6)) and the order cache depend on the frames before; every row starts from a freshly set volume and
transfer function (no resident copy, no cached mapping, no recorded order) and default settings.  The frames go through the synchronous
entry points on the context's own stream, a few through render_volume_device followed by a device synchronisation: which frames have
completed then does not depend on timing.  A refused frame is ["refused", code].

The fixture is what the commit BEFORE launch_frame was restated printed (scripts/feature_launch_plans.py test_gpu_composite_plans, with
--check: two contexts, no differing field); it is never taken from the code under test.

Not covered: the branches that run after a copy build is refused by the HBM guard or by allocation (the degradation to the quad copy, to
a resident copy, to the linear array; the dual pair that loses one copy) — a 16 x 20 x 24 volume cannot reach them."""
import json
import os

import numpy as np
import pytest

from gpu_feature import load, reset_context
from helpers import GOLDEN_DIR
from mip_helpers import ramp_tf
from plan_helpers import FIELDS, LIGHT, VOXELS, assert_same, axis_view, frame_params, launched, volume

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN_DIR, "composite_launch_plans.json")
ROW_FIELDS = FIELDS + ("copies", "aligned_copies")
SMALL, BIG, SLICED = (48, 32), (256, 128), (512, 512)      # one block of tiles and no order; 8 x 8 tiles: the smallest grid the order cache and the
                                                           # per-block run-copy choice accept; 1 MiB of pixels: vr_hip_render's two row slices
MODES = {"full": (0, 1.0), "ert": (0, 0.95), "esl": (1, 0.95)}        # mode -> (esl, ray_threshold)
CLIP = dict(box_min=(-0.75, -1.0, -0.5), box_max=(0.5, 0.75, 1.0), plane=(0.6, 0.0, 0.8, 0.1))
AXIS_VIEWS = ("x", "y", "z", "x_wide", "y_wide", "z_wide")
RUN_VIEWS = ("oblique", "persp_x", "persp_y", "persp_z", "persp_oblique", "pose180")
SOME_VIEWS = ("x", "oblique", "persp_x")                   # one axis view, one oblique view, one perspective view
STATES = ("clip", "lighting", "preint", "shadow", "backdrop")


def views(vr, window):
    """Orthogonal along x, y and z (built by hand: exact zeros) at two pixel pitches — 0.045: a wave's rectangle of cell columns fits its 64
    lanes (span product <= 64: the voxel windows); 0.08 (`_wide`): it does not (the quad-element windows) —, perspective along each axis,
    the oblique pose orthogonal and in perspective, and pose (180, 90, 0), whose direction carries rounding noise"""
    out = {}
    for name, axis in (("x", 0), ("y", 1), ("z", 2)):
        out[name] = axis_view(vr, window, axis, 0)
        out[name + "_wide"] = axis_view(vr, window, axis, 0, 0.08)
        out["persp_" + name] = axis_view(vr, window, axis, 1)
    out["oblique"] = vr.custom_view(window[0], window[1], 0, (-45.0, -45.0, 0.0), 2.0)
    out["persp_oblique"] = vr.custom_view(window[0], window[1], 1, (-45.0, -45.0, 0.0), 2.0)
    out["pose180"] = vr.custom_view(window[0], window[1], 0, (180.0, 90.0, 0.0), 2.0)
    return out


def row(view, sampling=1, mode="full", reps=2, window=BIG, kd=0.7, entry="volume", released=False, **settings):
    return dict(view=view, sampling=sampling, mode=mode, reps=reps, window=window, kd=kd, entry=entry, released=released, settings=settings)


# ---- the enumeration: each axis alone against the defaults, and the crossings named; {group: [(key, row)]} -----------------------------

def rows_views():
    for window in (SMALL, BIG):
        for view in AXIS_VIEWS + RUN_VIEWS:
            for sampling in (0, 1, 2):
                for mode in MODES:
                    yield f"{window[0]}/{view}/s{sampling}/{mode}", row(view, sampling, mode, reps=4, window=window)


def rows_layout():
    for view in AXIS_VIEWS + RUN_VIEWS:
        for sampling in (0, 1):
            for mode in ("full", "esl"):
                yield f"l0/{view}/s{sampling}/{mode}", row(view, sampling, mode, layout=0)


def rows_wide():
    for wide in (1, 2, 4):
        for view in SOME_VIEWS + ("persp_z",):
            for sampling in (0, 1):
                for mode in ("full", "esl"):
                    yield f"w{wide}/{view}/s{sampling}/{mode}", row(view, sampling, mode, wide=wide)


def rows_plane():
    for plane in range(10):
        for view in ("x", "z_wide", "oblique", "persp_x", "persp_oblique", "pose180"):
            for sampling in (0, 1):
                yield f"p{plane}/{view}/s{sampling}", row(view, sampling, reps=6 if plane in (6, 7) else 2, plane=plane)


def rows_column_copy():
    for copy in (0, 1, 2):
        for view in AXIS_VIEWS:
            for kd in (0.7, 0.0):
                for sampling in (0, 1):
                    yield f"c{copy}/{view}/kd{kd}/s{sampling}", row(view, sampling, kd=kd, column_copy=copy)


def rows_run_flavour():
    for flavour in (0, 1, 2):
        for view in RUN_VIEWS:
            for mode in ("full", "esl"):
                yield f"f{flavour}/{view}/{mode}", row(view, mode=mode, run_flavour=flavour)


def rows_mapping():
    for view in SOME_VIEWS:
        for sampling in (0, 1):
            for mode in ("full", "esl"):
                yield f"m9/{view}/s{sampling}/{mode}", row(view, sampling, mode, mapping=(1 + 4 * 2, 3, 5))


def rows_scheduling():
    for scheduling in (0, 1, 2):
        for view in SOME_VIEWS:
            for mode in MODES:
                yield f"t{scheduling}/{view}/{mode}", row(view, mode=mode, reps=4, scheduling=scheduling)


def rows_state():
    for state in STATES:
        for view in SOME_VIEWS + ("persp_z",):
            for sampling in (1, 2):
                for mode in ("full", "esl"):
                    yield f"{state}/{view}/s{sampling}/{mode}", row(view, sampling, mode, **{state: True})
        yield f"{state}/x/s0/full", row("x", 0, **{state: True})          # NEAREST: refused by every state but the clip
    yield "clip/oblique/s0/full", row("oblique", 0, clip=True)


def rows_released():
    for plane in (-1, 1):
        for view in ("x", "oblique", "persp_z"):
            for sampling in (0, 1, 2):
                for mode in ("full", "esl"):
                    yield f"p{plane}/{view}/s{sampling}/{mode}", row(view, sampling, mode, released=True, plane=plane)


def rows_sliced():
    for view in SOME_VIEWS:
        for mode in MODES:
            yield f"{view}/{mode}", row(view, mode=mode, reps=3, window=SLICED)


def rows_device():
    for view in SOME_VIEWS:
        for mode in MODES:
            yield f"{view}/{mode}", row(view, mode=mode, reps=4, entry="device")


GROUPS = {"views": (rows_views, 2 * 12 * 3 * 3), "layout": (rows_layout, 12 * 2 * 2), "wide": (rows_wide, 3 * 4 * 2 * 2), "plane": (rows_plane, 10 * 6 * 2),
          "column_copy": (rows_column_copy, 3 * 6 * 2 * 2), "run_flavour": (rows_run_flavour, 3 * 6 * 2), "mapping": (rows_mapping, 3 * 2 * 2),
          "scheduling": (rows_scheduling, 3 * 3 * 3), "state": (rows_state, 5 * (4 * 2 * 2 + 1) + 1), "released": (rows_released, 2 * 3 * 3 * 2),
          "sliced": (rows_sliced, 3 * 3), "device": (rows_device, 3 * 3)}


# ---- one row ---------------------------------------------------------------------------------------------------------------------------------

def defaults(vr, gpu):
    reset_context(vr, gpu)
    gpu.set_column_copy(0)
    gpu.set_run_flavour(0)


def apply(vr, gpu, layout=1, wide=0, plane=-1, column_copy=0, run_flavour=0, mapping=None, scheduling=1, clip=False, lighting=False, preint=False,
          shadow=False, backdrop=False):
    """the settings of a row, over the defaults (backdrop is the entry point's business)"""
    if layout != 1:
        gpu.set_layout(layout)
    gpu.set_wide_addressing(wide)
    gpu.set_brick_plane(plane)
    gpu.set_column_copy(column_copy)
    gpu.set_run_flavour(run_flavour)
    if mapping is not None:
        gpu.set_tile_mapping(*mapping)
    gpu.set_tile_scheduling(scheduling)
    if clip:
        gpu.set_clip(**CLIP)
    if lighting:
        gpu.set_lighting()
    if preint:
        gpu.set_preintegration(True)
    if shadow:
        gpu.set_shadow(LIGHT, dims=8, step=0.05)


def run_row(vr, gpu, voxels, r):
    """the row's repetitions: per frame the ROW_FIELDS, or the status of the refusal"""
    import torch
    w, h = r["window"]
    load(gpu, volume(voxels), ramp_tf(), window=r["window"])
    defaults(vr, gpu)
    if r["released"]:
        gpu.prepare()
        gpu.release_linear_copy()
    apply(vr, gpu, **r["settings"])
    esl, threshold = MODES[r["mode"]]
    p = frame_params(vr, views(vr, r["window"])[r["view"]], r["sampling"], esl, threshold, r["kd"])
    target = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda") if r["entry"] == "device" else None
    out = []
    for _ in range(r["reps"]):
        try:
            if r["settings"].get("backdrop"):
                gpu.render_backdrop(p, np.full((h, w, 4), 40, np.uint8), np.full((h, w), 2.5, np.float32))
            elif r["entry"] == "device":
                gpu.render_volume_device(p, target.data_ptr())
                torch.cuda.synchronize()
            else:
                gpu.render_volume(p)
        except vr.VrError as e:
            out.append(["refused", e.code])
            continue
        out.append(launched(gpu) + [int(gpu.volume_info().copies), gpu.run_aligned_info()["copies"]])
    return out


def group_plans(vr, gpu, voxels, group):
    """{key: row} of one group; the context is left on its defaults, with the linear array resident"""
    out = {}
    try:
        for key, r in GROUPS[group][0]():
            out[f"{voxels}/{group}/{key}"] = run_row(vr, gpu, voxels, r)
    finally:
        gpu.set_volume(volume(voxels))
        defaults(vr, gpu)
    return out


def record(vr, gpu):
    """everything the fixture holds"""
    plans = {}
    for voxels in VOXELS:
        for group in GROUPS:
            plans.update(group_plans(vr, gpu, voxels, group))
    return {"fields": list(ROW_FIELDS), "plans": plans}


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        data = json.load(f)
    assert tuple(data["fields"]) == ROW_FIELDS
    return data["plans"]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("voxels", VOXELS)
def test_plans_of_every_setting(vr, gpu, fixture, voxels, group):
    got = group_plans(vr, gpu, voxels, group)
    assert len(got) == GROUPS[group][1], len(got)
    assert_same(got, fixture, f"{voxels}/{group}/")


def test_the_fixture_reaches_every_decision(fixture):
    """a condition on the enumeration, held on the fixture itself: a thinned fixture fails"""
    assert len(fixture) == 2 * sum(count for _, count in GROUPS.values())
    frames = [f for reps in fixture.values() for f in reps]
    assert any(f[0] == "refused" for f in frames)
    ran = [dict(zip(ROW_FIELDS, f)) for f in frames if f[0] != "refused"]

    def values(field, of=ran):
        return {f[field] for f in of}
    assert values("layout") == set(range(8))
    assert values("column_voxels", [f for f in ran if f["layout"] == 7]) == {0, 1}
    assert values("column_shade_pairs") == {0, 1}
    assert values("run_flavour") == {0, 1, 2}
    assert values("clamp_fetch") == {0, 1}
    assert values("ordered") == {0, 1}
    assert {f["lane_map"] >> 2 for f in ran} == {0, 1, 2}
    assert values("shadowed") == {0, 1}
    # the measured validator of the per-tile run-copy choice: frames 0-3 on one run copy each, the per-tile choice from frame 4 on
    assert [f[0] for f in fixture["u8/plane/p6/oblique/s1"]] == [2, 3, 2, 3, 6, 6]
