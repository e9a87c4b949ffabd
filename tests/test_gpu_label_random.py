"""Random and holed parity of the labelled composite frames (vr_hip_render_labelled*): the random frames and the holed scenes of
tests/feature_random.py — frames of 1 x 8 to 69 x 49 pixels, cameras inside the cube, exact zeros in the direction, the four-fold ray step,
random transfer functions with holes and leading zeros, a slab of exact zeros through the volume, a random clip, block grid and threshold,
layout and wide addressing alternating per scene — with one uniform random label per voxel and the table of the five entry kinds, the
shading cycling through the cue, the frame's lighting, its shadow and both: held byte for byte, no tolerance anywhere, against label_render
of tests/label_ref.c.
Other seeds: VR_TEST_SEED=... pytest -m gpu tests/test_gpu_label_random.py"""
import pytest

import feature_random as fr
from gpu_feature import load, reset_context
from label_helpers import LabelRef, check, random_case, random_labels, set_state, table

pytestmark = pytest.mark.gpu

LABEL_STREAM = 9                                        # the generator stream of these scenes (0-8 are taken by the other feature files)
WINDOW = (70, 50)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout, a forced path or a table behind"""
    yield
    reset_context(vr, gpu)
    gpu.set_label_table(None)


@pytest.mark.parametrize("which", ("random", "holed"))
def test_frames_equal_the_restatement(vr, gpu, oracle, which):
    ref = LabelRef.instance()
    entries = table()
    scenes = fr.random_scenes(oracle, vr, LABEL_STREAM) if which == "random" else fr.holed_scenes(oracle, vr)
    frames = pixels = 0
    start = gpu.labelled_frames()
    for s, scene in enumerate(scenes):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene.vox, scene.tf, scene.esl, WINDOW)
        labels = random_labels(scene.vox, 10 + s)
        gpu.set_labels(labels)
        gpu.set_label_table(entries)
        for i, f in enumerate(scene.frames):
            case = random_case(scene, i, f, (s + i) % 4)
            case.what = case.what + ("layout", scene.layout, "wide", scene.wide)
            set_state(gpu, case)
            want = check(gpu, ref, case, labels, entries)
            frames, pixels = frames + 1, pixels + int(want.frame[..., 3].astype(bool).sum())
    print(f"{which}: {frames} frames, {pixels} pixels with alpha compared")
    assert frames == sum(len(s.frames) for s in scenes) and pixels > 20 * frames and gpu.labelled_frames() == start + frames, (frames, pixels)
