"""GPU tier of the float64 model (tests/f64_model.py): the kernels of the MIP, the section frames, the depth frames and picks, and the
labelled, tf2d and fused composites are held against the double-precision model DIRECTLY, not through their restatements — an edit that
changes a kernel and its restatement together still meets this file.  The scenes, views and arguments are those of
tests/test_f64_model.py without the random scenes (tests/f64_tier.py): per scene one context load and, per view and sampling, the MIP, the
four section modes with the depth buffer (one through the grey window), the three depth modes with all three buffers, one vr_hip_pick call
of 64 pixels, one labelled, one tf2d and two fused frames (SUM and OVER) — through the host entry points the other feature files use.  The
model's answers are computed here by numpy; the tolerances are the CPU tier's, measured on the model alone."""
import importlib

import pytest

import f64_tier as ft
from gpu_feature import reset_context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(vr):
    """a renderer of this module's own on cuda:0 with the faces of both add-on modules (tf2d and fusion), closed at the end"""
    import torch  # noqa: F401  (loads the process's HIP runtime first)
    fusion, tf2d = (importlib.import_module("volume-rendering_amd." + m) for m in ("fusion", "tf2d"))

    class TierRenderer(fusion.FusedRenderer, tf2d.Tf2dRenderer):
        pass
    r = TierRenderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole module: no test leaves a state, a table, labels or a second field behind"""
    yield
    reset_context(vr, gpu)
    gpu.clear_second_volume()
    gpu.clear_tf2d()
    gpu.clear_labels()
    gpu.set_label_table(None)


@pytest.mark.parametrize("name", ft.FIXED_NAMES)
def test_kernels_agree_with_the_model(vr, gpu, oracle, golden, name):
    """On the non-fragile hit pixels: the hit flag is the model's, every float the entry point returns lies within its tolerance, every
    byte within floor(256 t) + 1 of the model's; a fragile pixel is a hit or a miss as one of the model's two evaluations has it."""
    scene = ft.scene_named(vr, oracle, golden, name)
    tallies, frames = {}, 0
    try:
        ft.load_scene(gpu, scene)
        for job in ft.tier_jobs(vr, scene):
            job.on_device = True                        # (the picks: the 64 pixels of one call)
            tallies.setdefault(job.feature, ft.Tally()).add(ft.compare(job, job.gpu(gpu), (gpu.last_launch(),)))
            frames += 1
    finally:
        scene.cache.clear()
    wrong = []
    for feature, t in tallies.items():
        print(f"{name} {feature}: hit {t.hit}, fragile {t.fragile}, compared {t.compared}, worst " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(t.worst.items())))
        wrong += t.wrong
        assert t.compared >= (100 if feature == "pick" else ft.MIN_COMPARED), (name, feature, t.compared)
    assert frames == 78 and len(tallies) == 13 and not wrong, wrong[:10]
