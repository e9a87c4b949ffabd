"""Test-side helpers of the pre-integration tests: slab_render and slab_build_integral of tests/feature_ref.c (the slab-classified
composite frame of include/vr_hip.h vr_hip_set_preintegration, restated with the CPU oracle's own statics; tests/ref_library.py loads
it), and the volumes, transfer functions and views both tiers use."""
import ctypes as C

import numpy as np

from clip_helpers import IDENTITY, composite_params
from helpers import axis_view
from light_helpers import lit_views, lit_volumes
from mip_helpers import ramp_tf
from ref_library import Ref, SceneArgs, frame_array, ptr

POINT, SLAB, SLAB_DOUBLE, SLAB_SKIPPED_IS_NONE = 0, 1, 2, 3      # the `mode` of slab_render; the last is a wrong reading (sensitivity)
# what the GPU tier renders; on the plateau whole waves skip the empty samples in front of the block, and the first block sample needs the
# coordinate of a skipped one; on the ramp volume a peak three entries wide lies between consecutive samples
SLAB_VOLUMES = ("bucky", "blob_40x24x56", "random_u16", "plateau", "ramp")
_VIEW_VOLUME = {"ramp": "bucky"}                    # whose alternation of the two frame sizes a volume without one takes
# a clip whose cut face lies in dense matter: the first sample of a ray sits inside a gradient (Bucky's cage, the blob's flank)
DENSE_CUT = (None, None, (0.0, 0.0, 1.0, 0.13))


def ramp_volume():
    """x = 24, y = 8, z = 64, u8: v = clip(3 z + 5 x, 0, 255)"""
    z, y, x = np.mgrid[0:64, 0:8, 0:24]
    v = np.clip(3 * z + 5 * x, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(v)


def peak_tf():
    """zero but for entries 60, 61, 62 with alpha 0.45, 0.9, 0.45 and colour (a, a / 2, a / 4, a): premultiplied"""
    tf = np.zeros((128, 4), np.float32)
    for i, a in ((60, 0.45), (61, 0.9), (62, 0.45)):
        tf[i] = (a, a / 2, a / 4, a)
    return tf


def holed_tf():
    """the ramp transfer function with holes: entries 0..9, 40..49 and 100..104 are zero (leading zeros, and slabs that end in a hole)"""
    tf = ramp_tf().copy()
    tf[0:10] = 0
    tf[40:50] = 0
    tf[100:105] = 0
    return tf


def slab_volumes(golden):
    v = lit_volumes(golden)
    v["ramp"] = ramp_volume()
    return v


def slab_views(vr, golden, name):
    return lit_views(vr, golden, _VIEW_VOLUME.get(name, name))


def slab_scene(vr, golden, oracle, volumes, name, view, sampling, full_march, step_factor=1):
    """(voxels, params, tf, esl) of a volume's composite frame; the ramp volume takes the peak transfer function without empty blocks;
    step_factor 4 = the four-fold ray step, which selects the clamping kernel variant"""
    vox = volumes[name]
    p, tf, esl = composite_params(vr, golden, oracle, name, vox, view, sampling, full_march)
    if name == "ramp":
        tf, esl = peak_tf(), np.zeros(1024, np.uint32)      # no block is marked empty: the default mode of this volume only terminates early
    if step_factor != 1:
        p = p.copy()
        p.ray_step = float(np.float32(p.ray_step) * np.float32(step_factor))
    return vox, p, tf, esl


def phase_scene(vr, sampling):
    """The phase-independence scene: the ramp volume under the peak transfer function viewed along z at step 0.1, no leaping, no cue.
    Returns (voxels, params, tf, esl, window): window = the rows and columns of the frame whose rays cross the whole peak."""
    vox = ramp_volume()
    p = vr.VrParams()
    p.view = axis_view(vr, (24, 8, 64), 2, 1, cells_per_pixel=0.5, margin=0)
    p.ray_step, p.ray_threshold, p.light_kd, p.esl, p.esl_block_dims = 0.1, 0.95, 0.0, 0, 1
    for j in range(3):
        p.esl_block_size[j] = 2.0
    p.sampling = sampling
    return vox, vr.whole_frame(p), peak_tf(), np.zeros(1024, np.uint32), (slice(4, -4), slice(4, 36))


class SlabRef(Ref):
    """slab_render / slab_build_integral of tests/feature_ref.c; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.L.slab_render.restype = C.c_int
        self.L.slab_build_integral.restype = None

    def integral(self, tf):
        """K of the 128 premultiplied entries: [128, 4] float32"""
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        out = np.zeros((128, 4), np.float32)
        self.L.slab_build_integral(ptr(tf), ptr(out))
        return out

    def render(self, params, voxels, tf, esl, mode=SLAB, clip=IDENTITY, lighting=None, q=None, strength=1.0, counters=False):
        """the composite frame (TRILINEAR modes) under `clip`, with the reference's cue (lighting None) or lit by `lighting` = (ambient,
        diffuse, specular, shininess_log2), scaled by the light grid q (None: no shadow); mode POINT / SLAB / SLAB_DOUBLE / SLAB_SKIPPED_IS_NONE.
        counters=True: (frame, samples of the accumulation loop, wide-slab samples, narrow-slab samples)"""
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength, mode)

        def make():
            out, cnt = frame_array(params, 4), (C.c_uint64 * 3)()
            assert self.L.slab_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, a.mode, ptr(out), cnt) == 0
            return out, int(cnt[0]), int(cnt[1]), int(cnt[2])
        out = self.cached(("frame",) + a.key, a.keep, make)
        return out if counters else out[0]
