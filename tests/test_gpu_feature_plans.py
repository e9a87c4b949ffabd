"""What the host decides for the five kinds of frame that go through launch_full_march_frame (vr_hip_api.cpp) — MIP, isosurface, section,
depth, labelled —, pinned: the layout, the chunk plane, the lane order, the tile phases, the tile grid and the straddle figure that
vr_hip_last_launch reports, and the run flavour beside them, of tiny frames under every setting the decision branches on, held against
tests/golden/feature_launch_plans.json.  Every copy of a volume gives the same pixels, so the parity tiers do not see a frame that reads
another copy or maps its tiles differently; this file does.  The fixture is what the commit BEFORE the launchers were restated printed
(scripts/feature_launch_plans.py prints it; it is never taken from the code under test); the plan is host arithmetic, so every field of
last_launch() is compared, none left out."""
import json
import os

import numpy as np
import pytest

from gpu_feature import load, reset_context
from helpers import GOLDEN_DIR
from mip_helpers import ramp_tf
from plan_helpers import FIELDS, LIGHT, VOXELS, assert_same, axis_view, frame_params, launched, volume

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN_DIR, "feature_launch_plans.json")
WINDOW = (48, 32)
KINDS = {"mip": (0, 1, 2), "iso": (1, 2), "section": (1, 2), "depth": (1, 2), "labelled": (1, 2)}      # kind -> its legal sampling modes
CLIP = dict(box_min=(-0.75, -1.0, -0.5), box_max=(0.5, 0.75, 1.0), plane=(0.6, 0.0, 0.8, 0.1))


def views(vr):
    """orthogonal along x, y and z (built by hand: exact zeros), one oblique orthogonal pose, one perspective view along z"""
    out = {name: axis_view(vr, WINDOW, axis, perspective) for name, axis, perspective in (("x", 0, 0), ("y", 1, 0), ("z", 2, 0), ("persp_z", 2, 1))}
    out["oblique"] = vr.custom_view(WINDOW[0], WINDOW[1], 0, (-45.0, -45.0, 0.0), 2.0)
    return out


def plan(vr, gpu, kind, p, top):
    """the frame of `kind`, and what it launched: the FIELDS of last_launch(), or the status of the refusal"""
    try:
        if kind == "mip":
            gpu.render_mip(p)
        elif kind == "iso":
            gpu.render_iso(p, 0.4 * top, depth=True)
        elif kind == "section":
            gpu.render_section(p, (0.3, 0.5, 0.8, 0.05), 0.2, "mean", depth=True)
        elif kind == "depth":
            gpu.render_depth(p, 0.3, "first", value=True)
        else:
            gpu.render_labelled(p)
    except vr.VrError as e:
        return ["refused", e.code]
    return launched(gpu)


def load_volume(gpu, voxels):
    vox = volume(voxels)
    load(gpu, vox, ramp_tf(), window=WINDOW)
    gpu.set_labels((np.arange(vox.size, dtype=np.uint32).reshape(vox.shape) % 5).astype(np.uint8))
    return vox, float(np.iinfo(vox.dtype).max)


def frames_of(vr, names=None, esls=(1, 0)):
    """(key, kind, params) of every kind x sampling x view; esl on, and for the two kinds that skip by block maxima also off"""
    for name, view in views(vr).items():
        if names is not None and name not in names:
            continue
        for kind, samplings in KINDS.items():
            for sampling in samplings:
                for esl in (esls if kind in ("mip", "iso") else esls[:1]):
                    yield f"{name}/{kind}/s{sampling}/e{esl}", kind, frame_params(vr, view, sampling, esl)


def sweep(vr, gpu, voxels):
    """{key: plan}: layout x wide addressing x forced plane over every frame without a clip, and layout x clip on at the context's own
    addressing and plane; the context is left on its defaults"""
    _, top = load_volume(gpu, voxels)
    out = {}
    try:
        for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
            gpu.set_layout(layout)
            for wide in (0, 1, 2):
                gpu.set_wide_addressing(wide)
                for plane in (-1, 0, 1, 2):
                    gpu.set_brick_plane(plane)
                    for key, kind, p in frames_of(vr):
                        out[f"{voxels}/l{layout}/w{wide}/p{plane}/clip0/{key}"] = plan(vr, gpu, kind, p, top)
            gpu.set_wide_addressing(0)
            gpu.set_brick_plane(-1)
            gpu.set_clip(**CLIP)
            for key, kind, p in frames_of(vr):
                out[f"{voxels}/l{layout}/w0/p-1/clip1/{key}"] = plan(vr, gpu, kind, p, top)
            gpu.clear_clip()
    finally:
        reset_context(vr, gpu)
    return out


def released(vr, gpu):
    """{key: plan} of the 1-byte volume with every copy prepared and the linear array released; the volume is set again on the way out"""
    vox, top = load_volume(gpu, "u8")
    out = {}
    try:
        gpu.prepare()
        gpu.release_linear_copy()
        for plane in (-1, 1):
            gpu.set_brick_plane(plane)
            for key, kind, p in frames_of(vr, ("x", "oblique", "persp_z")):
                out[f"released/p{plane}/{key}"] = plan(vr, gpu, kind, p, top)
    finally:
        gpu.set_volume(vox)
        reset_context(vr, gpu)
    return out


def record(vr, gpu):
    """everything the fixture holds"""
    plans = {}
    for voxels in VOXELS:
        plans.update(sweep(vr, gpu, voxels))
    plans.update(released(vr, gpu))
    return {"fields": list(FIELDS), "plans": plans}


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        data = json.load(f)
    assert tuple(data["fields"]) == FIELDS
    return data["plans"]


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    yield
    reset_context(vr, gpu)


@pytest.mark.parametrize("voxels", VOXELS)
def test_plans_of_every_setting(vr, gpu, fixture, voxels):
    got = sweep(vr, gpu, voxels)
    assert len(got) == 2 * (3 * 4 + 1) * 5 * 16 and not any(v[0] == "refused" for v in got.values()), len(got)
    assert_same(got, fixture, voxels + "/")


def test_plans_with_the_linear_array_released(vr, gpu, fixture):
    got = released(vr, gpu)
    assert len(got) == 2 * 3 * 16, len(got)
    assert_same(got, fixture, "released/")


def test_a_shadow_builds_once_and_leaves_the_labelled_plan(vr, gpu, fixture):
    _, top = load_volume(gpu, "u8")
    start = gpu.shadow_builds()[0]
    gpu.set_shadow(LIGHT, dims=8, step=0.05)
    for key, kind, p in frames_of(vr, ("x", "oblique")):
        if kind == "labelled":
            assert plan(vr, gpu, kind, p, top) == fixture[f"u8/l1/w0/p-1/clip0/{key}"], key
    assert gpu.shadow_builds()[0] == start + 1


@pytest.mark.parametrize("forced", (-1, 1))
def test_a_labelled_frame_leaves_the_forced_plane(vr, gpu, fixture, forced):
    """1-byte voxels: a labelled frame reads the (x,y) quad copy whatever the view.  The MIP frame behind it — behind one that ran, and
    behind one that pre-integration refuses — has the plan of the fixture: along x the (y,z) plane, or the plane forced"""
    _, top = load_volume(gpu, "u8")
    gpu.set_brick_plane(forced)
    frames = {key: (kind, p) for key, kind, p in frames_of(vr, ("x",))}
    for preint in (False, True):
        gpu.set_preintegration(preint)
        got = plan(vr, gpu, *frames["x/labelled/s1/e1"], top)
        assert got == (["refused", 1] if preint else fixture[f"u8/l1/w0/p{forced}/clip0/x/labelled/s1/e1"]), (preint, got)
        gpu.clear_preintegration()
        for key in ("x/mip/s1/e1", "x/mip/s2/e0"):
            assert plan(vr, gpu, *frames[key], top) == fixture[f"u8/l1/w0/p{forced}/clip0/{key}"], (preint, key)
