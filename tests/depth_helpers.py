"""Test-side helpers of the depth tests: depth_render of tests/depth_ref.c (the depth frames of include/vr_hip.h vr_hip_render_depth /
vr_hip_pick, restated with the CPU oracle's own statics on top of tests/feature_ref.c), built through ref_library.compile_test_library,
the opacities and the frame list both tiers walk, and what the GPU tiers do with one frame (check, classify, depth_launch).
The `cmode` of DepthRef.render is slab_helpers' POINT or SLAB — and SLAB_SKIPPED_IS_NONE, slab_colour's wrong reading "a sample the
library may skip unresolved counts as no predecessor", which depth_render passes to slab_colour unchanged: the sensitivity of the holed
scenes of tests/feature_random.py (tests/test_depth_random_model.py)."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import CLIPS, IDENTITY
from gpu_feature import depth_diff
from light_helpers import LIT_VOLUMES, PHONG, lit_views
from ref_library import Ref, SceneArgs, compile_test_library, frame_array, ptr
from slab_helpers import POINT, SLAB, slab_scene

DEPTH_VOLUMES = LIT_VOLUMES                             # bucky, blob_40x24x56, random_u16, plateau
MODES = ("first", "peak", "mean")
MODE_NUMBER = {"first": 0, "peak": 1, "mean": 2}
ACC_BEFORE, TERMINATOR_LOST, MEAN_BY_ALPHA, PEAK_LAST = 1, 2, 3, 4       # the `perturb` of depth_render: the sensitivity test's wrong readings
MISS, CLIPPED = 0xffffffff, 0xfffffffe
LIGHTING = PHONG                                        # what the lit composite frames of the alpha tie are lit by

# Two opacities per volume, chosen from the restatement alone: tests/test_depth_model.py asserts the conditions of the issue on them and
# prints the shares.  The low one lies below the final alpha of most rays that composite anything, so that FIRST carries nearly the surfaces
# PEAK and MEAN carry; the high one lies above the final alpha of the thin rays and below the default mode's ray_threshold, so that FIRST
# loses surfaces that PEAK and MEAN keep and its surfaces lie deep, away from the peak.  PEAK and MEAN do not look at the opacity: a ray
# has a surface in them where it has composited anything at all.
# Shares found over each volume's list (36 frames: both samplings), per opacity.  "of the rays": of the rays that hit the cube [-1, 1]^3 —
# under the box and the plane many of them are clipped away, which is why even the random volume has rays without a surface in every mode —;
# "of the segments": of those that keep a segment under the clip; FIRST != PEAK: of the pixels with a surface in both.
#   volume          opacity   surface, of the rays: FIRST / PEAK = MEAN    of the segments: FIRST / PEAK    FIRST != PEAK    wide-slab samples
#   bucky           0.1       0.391 / 0.405                               0.657 / 0.680                    0.520            398253
#                   0.9       0.170 / 0.405                               0.285 / 0.680                    0.997
#   blob_40x24x56   0.1       0.285 / 0.299                               0.476 / 0.499                    0.418            623975
#                   0.7       0.129 / 0.299                               0.216 / 0.499                    0.531
#   random_u16      0.3       0.593 / 0.599                               0.990 / 0.999                    0.102            662099
#                   0.9       0.509 / 0.599                               0.849 / 0.999                    0.990
#   plateau         0.1       0.199 / 0.200                               0.334 / 0.335                    0.277            41477
#                   0.9       0.149 / 0.200                               0.250 / 0.335                    1.000
OPACITIES = {"bucky": (0.1, 0.9), "blob_40x24x56": (0.1, 0.7), "random_u16": (0.3, 0.9), "plateau": (0.1, 0.9)}

_CLIP_CYCLE = (IDENTITY, CLIPS["box"], CLIPS["plane"], CLIPS["both"])
_CLIP_NAMES = ("identity", "box", "plane", "both")

_library = None


def depth_library():
    """tests/depth_ref.c as a loaded library, built on first use"""
    global _library
    if _library is None:
        tmp = tempfile.mkdtemp(prefix="depth_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _library = compile_test_library(tmp, "depth_ref.c", "libdepth_ref.so")
    return _library


class DepthFrame:
    """depth_render's answers for one frame: depth, value, alpha (float32 frames), count (samples of the accumulation loop per pixel; 0: a ray
    whose segment is leapt over entirely, CLIPPED: a ray that hits the cube and is clipped away, MISS: a ray that misses the cube), last (k of
    the loop's last sample, NaN where there is none), terminated (that sample ended the ray by acc > ray_threshold), pick (position xyz and voxel index xyz per pixel), wide (wide-slab samples)"""

    def __init__(self, depth, value, alpha, count, last, pick, wide):
        self.depth, self.value, self.alpha, self.count, self.pick, self.wide = depth, value, alpha, count, pick, wide
        self.last, self.terminated = np.abs(last), np.signbit(last) & ~np.isnan(last)
        self.rays = count != MISS                       # rays that hit the cube
        self.segment = self.rays & (count != CLIPPED)   # ... and keep a segment under the clip
        self.surface = depth >= 0.0


class DepthRef(Ref):
    """depth_render of tests/depth_ref.c on WHOLE frames; cached per argument set.  cmode: POINT, SLAB or SLAB_SKIPPED_IS_NONE."""

    def __init__(self):
        super().__init__()
        self.D = depth_library()
        self.D.depth_render.restype = C.c_int

    def render(self, params, voxels, tf, esl, opacity, mode="first", cmode=POINT, clip=IDENTITY, perturb=0):
        a = SceneArgs(params, voxels, tf, esl, clip, mode=cmode)

        def make():
            depth, value, alpha = (frame_array(params, dtype=np.float32) for _ in range(3))
            count, last, pick, wide = frame_array(params, dtype=np.uint32), frame_array(params, dtype=np.float32), frame_array(params, 6, dtype=np.float32), C.c_uint64(0)
            assert self.D.depth_render(*a.base, a.esl, a.clip, a.mode, C.c_float(opacity), C.c_uint32(MODE_NUMBER[mode]), C.c_uint32(perturb), ptr(depth), ptr(value),
                                       ptr(alpha), ptr(count), ptr(last), ptr(pick), C.byref(wide)) == 0
            return (DepthFrame(depth, value, alpha, count, last, pick, int(wide.value)),)
        return self.cached(("depth",) + a.key + (float(np.float32(opacity)), mode, int(perturb)), a.keep, make)[0]


def alpha_byte(alpha):
    """map_float_int(alpha, 256): (int) (alpha * 256.0f) clamped to 0..255"""
    scaled = (np.asarray(alpha, np.float32) * np.float32(256.0)).astype(np.float32)
    return np.clip(scaled.astype(np.int64), 0, 255).astype(np.uint8)


# ---- what the GPU tiers (tests/test_gpu_depth.py, tests/test_gpu_depth_random.py) do with one frame ----

def depth_launch(info):
    """what every depth frame's launch looks like: what a clipped MIP frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


def classify(gpu, cmode):
    if cmode == SLAB:
        gpu.set_preintegration()
    else:
        gpu.clear_preintegration()


def check(gpu, ref, what, vox, p, tf, esl, opacity, mode, cmode=POINT, clip=IDENTITY):
    """the host entry point with all three buffers (depth, value and alpha bits) against depth_render; returns the restatement's frame.
    The context's clip and classification are the caller's business."""
    want = ref.render(p, vox, tf, esl, opacity, mode, cmode, clip)
    depth, value, alpha = gpu.render_depth(p, opacity, mode, value=True, alpha=True)
    info = gpu.last_launch()
    wrong = depth_diff(depth, want.depth), depth_diff(value, want.value), depth_diff(alpha, want.alpha)
    assert wrong == (0, 0, 0), (what, opacity, mode, wrong, info)
    assert depth_launch(info), (what, info)
    assert (depth[depth != -1.0] >= 0.0).all(), (what, "every surface reads as a surface to a backdrop frame")
    return want


def tier_frames(vr, golden, oracle, volumes, name, sampling):
    """The scenes of both tiers' main tests for one (volume, sampling): the nine views of lit_views, two frames each with complementary
    settings — classification point / slab, leaping and early termination on / off (the default mode, threshold below 1 / the full march), the volume's ray
    step / four times it, and the clip (identity, box, plane, both) — arranged so that every pair of settings meets.
    Yields (what, voxels, params, tf, esl, clip, cmode); each is rendered in the three modes at both opacities of OPACITIES[name]."""
    for v, (label, view) in enumerate(lit_views(vr, golden, name)):
        cmode, leaping, fourfold = v % 2, (v // 2) % 2, (v // 4) % 2
        for second in (0, 1):
            c, e, f = (cmode ^ second), (leaping ^ second), (fourfold ^ second)
            k = (v + 2 * second) % 4
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, not e, 4 if f else 1)
            if e and p.ray_threshold >= 1.0:            # (the blob's golden state never terminates a ray: its default-mode frames take 0.95 here)
                p = p.copy()
                p.ray_threshold = 0.95
            yield (name, sampling, label, _CLIP_NAMES[k], "slab" if c else "point", "default" if e else "full", 4 if f else 1), vox, p, tf, esl, _CLIP_CYCLE[k], (SLAB if c else POINT)
