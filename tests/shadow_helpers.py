"""Test-side helpers of the shadow tests: shadow_build and shadow_render of tests/feature_ref.c (the light grid of include/vr_hip.h
vr_hip_set_shadow and the composite frame scaled by it, restated with the CPU oracle's own statics; tests/ref_library.py loads it), and
the lights, grids and scenes both tiers use."""
import ctypes as C

import numpy as np

from clip_helpers import IDENTITY
from ref_library import Ref, SceneArgs, clip_floats, frame_array, ptr, volume_args

LIGHTS = {"outside": (2.0, 1.5, -2.5), "top": (0.0, 0.0, 3.0), "inside": (0.2, -0.1, 0.3)}
CUTOFF = 1.0 / 256.0
COMPOSITE_VOLUMES = ("bucky", "blob_40x24x56", "random_u16")
# (volume, light, S) whose light grid the GPU tier downloads; the frames of FRAME_SCENES are rendered too.  Not among them, by the figures of
# the prototype: blob_40x24x56 with the inside light (99 % of the nodes black) and random_u16 with the outside light at S = 9 (no node between).
GRID_SCENES = (("bucky", "outside", 9), ("bucky", "top", 17), ("bucky", "inside", 33),
               ("blob_40x24x56", "outside", 17), ("blob_40x24x56", "top", 9), ("blob_40x24x56", "top", 33),
               ("shell48", "top", 17), ("shell48", "inside", 9), ("shell48", "outside", 33),
               ("random_u16", "top", 17), ("random_u16", "top", 33))
FRAME_SCENES = {"bucky": ("top", 17), "blob_40x24x56": ("outside", 17), "random_u16": ("top", 17)}
# S = 2: one cell, i = min(.., S - 2) = 0 everywhere.  The eight nodes are the cube's corners; with the outside light seven of them are 255 and
# one is 0 — no byte between, the situation the cap excludes — so the smallest grid takes the inside light, under which every corner's light
# ray ends inside Bucky and all eight bytes lie strictly between (tests/test_shadow_model.py holds it to the caps of the other scenes).
SMALLEST = ("bucky", "inside", 2)


class ShadowRef(Ref):
    """shadow_build / shadow_render of tests/feature_ref.c; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.L.shadow_build.restype = C.c_int
        self.L.shadow_render.restype = C.c_int

    def build(self, light, dims, step, voxels, tf, cutoff=CUTOFF, sampling=1, clip=None):
        """q as a (S, S, S) uint8 array indexed [z, y, x]; clip None = no clip set"""
        vox, volume = volume_args(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        lf = np.array(light, np.float32)
        cf = None if clip is None else clip_floats(clip)

        def make():
            q = np.zeros((dims, dims, dims), np.uint8)
            assert self.L.shadow_build(ptr(lf), C.c_uint32(dims), C.c_float(step), C.c_float(cutoff), C.c_uint32(sampling), *volume, ptr(tf), ptr(cf), ptr(q)) == 0
            return (q,)
        return self.cached(("q", lf.tobytes(), int(dims), float(np.float32(step)), float(np.float32(cutoff)), int(sampling), vox.ctypes.data, vox.shape,
                            tf.tobytes(), None if cf is None else cf.tobytes()), vox, make)[0]

    def render(self, params, voxels, tf, esl, q=None, strength=1.0, clip=IDENTITY):
        """the composite frame (TRILINEAR modes) scaled by the light grid q (None: no shadow) under `clip`"""
        a = SceneArgs(params, voxels, tf, esl, clip, q=q, strength=strength)

        def make():
            out = frame_array(params, 4)
            assert self.L.shadow_render(*a.base, a.esl, a.clip, *a.shadow, ptr(out)) == 0
            return (out,)
        return self.cached(("frame",) + a.key, a.keep, make)[0]


def unlit(params):
    """the same frame with light_kd = 0: no diffuse term, the shadow factor alone"""
    p = params.copy()
    p.light_kd = 0.0
    return p
