"""The pipelined per-lane march of the column kernels (col_lane_march in csrc/vr_kernels.hip): the waves that cannot take the column path
fetch DEPTH samples ahead of the one they composite.  Two ways into it, every frame byte for byte against the CPU oracle and with the launch
record of the kernel it claims to test (tests/test_column_edges.py's _check_frame):

  * natural mixed entry: on the orthogonal pose (180,90,0) one row of waves holds lanes whose kx differ by one ulp
    (scripts/lane_march_waves.py replays which; asserted here, so the frames do hold such waves) and marches per lane inside an otherwise
    ordinary column frame;
  * forced column frames (vr_hip_set_brick_plane(8)) of oblique orthogonal poses, where hardly a wave shares kx and the coordinate along
    the march axis: rays shorter than, as long as and just longer than the pipeline, lateral extents 1 - 9, a camera inside the cube, and a
    transfer function under which every sample composites.

The same frames once more under the bounds-checked build (every speculative fetch address held against its copy)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_feature import BOUNDS_LIB
from helpers import ColumnScene, column_params, smooth_noisy_volume, voxel_windows_fit
from test_column_edges import OBLIQUE_POSES, _check_frame, _open_tf, _oracle_frame, _policy_restored, _sample_ratio, _thin_base_tf, _what

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from lane_march_waves import mixed_entry_waves  # noqa: E402

LANE_DEPTH = 6                                  # kColLaneDepth (VR_COL_LANE_DEPTH) of csrc/vr_kernels.hip
BUFFER = 128
MIXED_POSE = (180.0, 90.0, 0.0)
FOUR_KERNELS = (("TRILINEAR lit", 1, 0.6), ("NEAREST lit", 0, 0.6))       # TRILINEAR: column-copy modes 0, 1, 2 = three kernels

_scenes = {}


def _shell_volume(shape_zyx):
    """a hollow ellipsoid: opaque wall, transparent inside and outside — rays cross two thin dense stretches with empty space between"""
    z, y, x = shape_zyx
    zz, yy, xx = np.mgrid[0:z, 0:y, 0:x].astype(np.float64)
    r = np.sqrt(sum(((g - 0.5 * (n - 1)) / (0.5 * n)) ** 2 for g, n in ((xx, x), (yy, y), (zz, z))))
    return np.clip(255.0 * np.exp(-((r - 0.62) / 0.12) ** 2), 0, 255).astype(np.uint8)


def _scene(oracle, kind, shape_zyx, tf_name="thin"):
    key = (kind, shape_zyx, tf_name)
    if key not in _scenes:
        vox = smooth_noisy_volume(shape_zyx, 20261019 + sum(shape_zyx)) if kind == "random" else _shell_volume(shape_zyx)
        # thin: the default opacity times 6 / edge (a ray through the smooth field reaches 0.95 part-way); the shell's two thin walls get
        # 16 / edge, or no ray would reach 0.95 at all
        base = _open_tf(oracle, shape_zyx) if tf_name == "open" else _thin_base_tf(oracle, shape_zyx, 6.0 if kind == "random" else 16.0)
        _scenes[key] = ColumnScene.synthetic(oracle, kind, vox, base, tf_name)
    return _scenes[key]


def _march_axis(p, dims):
    return int(np.argmax([abs(p.view.direction[j] * dims[j]) for j in range(3)]))


# ---- natural mixed entry -------------------------------------------------------------------------------------------------------------

NATURAL_VOLUMES = (("random", (32, 32, 32)), ("shell", (32, 32, 32)), ("random", (56, 24, 40)), ("shell", (56, 24, 40)))       # (z, y, x)
NATURAL_WAVES = {64: (8, 6), 128: (16, 13)}     # viewport -> (mixed-entry waves, their wave row), tile phase 0


@pytest.mark.parametrize("kind,shape", NATURAL_VOLUMES, ids=[f"{k}-{'x'.join(str(n) for n in s[::-1])}" for k, s in NATURAL_VOLUMES])
def test_lane_march_natural_mixed_entry(vr, gpu, oracle, kind, shape):
    """Pose (180,90,0) at 64 x 64 and 128 x 128 under the automatic policy: the waves of one wave row march per lane beside waves on the
    window path.  Lit, column-copy modes 0 / 1 / 2 and NEAREST, thresholds 1.0, 0.95 and 0.5 (lanes end while fetches are in flight)."""
    scene = _scene(oracle, kind, shape)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for w, (count, row) in NATURAL_WAVES.items():
            view = vr.custom_view(w, w, False, MIXED_POSE, 2.0)
            waves = mixed_entry_waves(view)
            assert len(waves) == count and {wy for _, wy, _ in waves} == {row}, (w, waves)
            for mode, sampling, kd in FOUR_KERNELS:
                for threshold in (1.0, 0.95, 0.5):
                    p = column_params(vr, scene, view, sampling, kd, threshold)
                    what = _what(scene, p, mode, f" pose {MIXED_POSE}")
                    if threshold < 1.0:
                        assert _sample_ratio(oracle, scene, p) < 1.0, what               # some ray does end early
                    _check_frame(vr, gpu, oracle, scene, p, what, voxel_windows=voxel_windows_fit(p, scene.dims, _march_axis(p, scene.dims)))
                    assert _oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


# ---- forced per-lane frames ------------------------------------------------------------------------------------------------------------

MARCH_EXTENTS = (1, 2, LANE_DEPTH, LANE_DEPTH + 1, LANE_DEPTH + 2)
LATERALS = {1: (5, 9), 2: (9, 3), LANE_DEPTH: (1, 7), LANE_DEPTH + 1: (8, 2), LANE_DEPTH + 2: (4, 6)}       # lateral extents 1 - 9, each once
POSE_IDS = ["-".join(f"{a:g}" for a in angles) for angles in OBLIQUE_POSES]


def _forced_shape(vr, angles, extent):
    """(z, y, x) with `extent` cells along the axis the pose looks along (its largest direction component) and LATERALS[extent] across"""
    d = vr.custom_view(16, 16, False, angles, 2.0).direction
    axis = int(np.argmax([abs(d[j]) for j in range(3)]))
    dims = list(LATERALS[extent])
    dims.insert(axis, extent)                                                    # x, y, z
    return tuple(dims[::-1])


def _forced_frames(vr, gpu, oracle, scene, angles, distance, w, thresholds):
    view = vr.custom_view(w, w, False, angles, distance)
    for mode, sampling, kd in FOUR_KERNELS:
        for threshold in thresholds:
            p = column_params(vr, scene, view, sampling, kd, threshold)
            what = _what(scene, p, mode, f" pose {angles} distance {distance:g} forced")
            _check_frame(vr, gpu, oracle, scene, p, what, voxel_windows=voxel_windows_fit(p, scene.dims, _march_axis(p, scene.dims)))
            yield p, what


@pytest.mark.parametrize("angles", OBLIQUE_POSES, ids=POSE_IDS)
def test_lane_march_forced_short_rays(vr, gpu, oracle, angles):
    """Forced column frames of slightly and strongly oblique poses over volumes of 1, 2, DEPTH, DEPTH + 1 and DEPTH + 2 cells along the
    view axis: a ray takes about as many samples as that, so the pipeline's prologue fetches past the end of every ray, exactly to it, or
    just short of it.  Open transfer function (no leading zero entry): every sample composites.  Thresholds 1.0 and 0.8."""
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        gpu.set_brick_plane(8)
        for extent in MARCH_EXTENTS:
            scene = _scene(oracle, "random", _forced_shape(vr, angles, extent), "open")
            scene.load(gpu)
            drawn = [_oracle_frame(oracle, scene, p)[0][..., 3].any() for p, _ in _forced_frames(vr, gpu, oracle, scene, angles, 2.0, 40, (1.0, 0.8))]
            assert any(drawn), f"{scene.vox.shape} pose {angles}: every oracle frame is empty"


@pytest.mark.parametrize("angles", OBLIQUE_POSES, ids=POSE_IDS)
def test_lane_march_forced_camera_inside_the_cube(vr, gpu, oracle, angles):
    """The same poses from inside the cube (0.4 before the centre and at it): kx = 0 for every lane, the coordinate along the march axis still
    differs from lane to lane, so the waves march per lane from the middle of their columns.  40 x 24 x 56 under the thin default transfer
    function (windows to skip, early termination at 0.8) and under the open one."""
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        gpu.set_brick_plane(8)
        for tf_name in ("thin", "open"):
            scene = _scene(oracle, "random", (56, 24, 40), tf_name)
            scene.load(gpu)
            for distance in (0.4, 0.0):
                for p, what in _forced_frames(vr, gpu, oracle, scene, angles, distance, 72, (1.0, 0.8)):
                    assert _oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


# ---- the same under the bounds-checked build ---------------------------------------------------------------------------------------------

def test_lane_march_under_the_bounds_checked_build():
    """Both groups once with build_variants/libvr_hip_bounds.so in a child process (VR_HIP_LIB): every frame still equals the oracle, and a
    speculative fetch address outside its copy would fail its frame (VrError).  The library is built here when it is missing."""
    if not os.path.exists(BOUNDS_LIB):
        subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), "bounds", "-DVR_BOUNDS_CHECK"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, VR_HIP_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "natural or forced"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
