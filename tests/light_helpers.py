"""Test-side helpers of the lighting tests: light_render of tests/feature_ref.c (the gradient-lit composite frame of include/vr_hip.h
vr_hip_set_lighting, restated with the CPU oracle's own statics; tests/ref_library.py loads it), and the lightings, volumes and views
both tiers use."""
import ctypes as C

import numpy as np

from clip_helpers import IDENTITY
from iso_helpers import all_volumes, views_of
from ref_library import Ref, SceneArgs, frame_array, ptr

# (ambient, diffuse, specular, shininess_log2)
PHONG = (0.25, 0.65, 0.4, 4)
IDENTITY_LIGHTING = (1.0, 0.0, 0.0, 4)              # fma(c, 1, (0 * sp) * c.w) = c: the bytes of the frame with light_kd = 0
LIGHTINGS = (PHONG, (0.0, 1.0, 0.0, 0), (0.0, 0.0, 1.0, 0), (0.0, 0.0, 1.0, 10))
# what the GPU tier renders; the plateau volume is the one on which the zero-gradient branch is taken (tests/test_light_model.py holds both)
LIT_VOLUMES = ("bucky", "blob_40x24x56", "random_u16", "plateau")
_VIEW_INDEX = {"bucky": 0, "blob_40x24x56": 1, "random_u16": 3, "plateau": 0}      # which of the two frame sizes view 0 takes (iso_helpers.views_of)


def plateau():
    """24^3 u8, zero but for [6, 18)^3 = 200: inside the block every central difference is 0"""
    v = np.zeros((24, 24, 24), np.uint8)
    v[6:18, 6:18, 6:18] = 200
    return v


def lit_volumes(golden):
    v = all_volumes(golden)
    v["plateau"] = plateau()
    return v


def lit_views(vr, golden, name):
    """the nine views of iso_helpers.views_of (eight benchmark views at 80 x 80 / 120 x 72 and the far perspective view)"""
    return views_of(vr, golden, _VIEW_INDEX[name])


def cue(params):
    """the same frame with light_kd = 0: no cue"""
    p = params.copy()
    p.light_kd = 0.0
    return p


class LightRef(Ref):
    """light_render of tests/feature_ref.c; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.L.light_render.restype = C.c_int

    def render(self, params, voxels, tf, esl, lighting, q=None, strength=1.0, clip=IDENTITY, counters=False):
        """the composite frame (TRILINEAR modes) lit by `lighting` = (ambient, diffuse, specular, shininess_log2), scaled by the light grid q
        (None: no shadow) under `clip`; counters=True: (frame, dense samples, dense samples with a zero gradient)"""
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength)

        def make():
            out, cnt = frame_array(params, 4), (C.c_uint64 * 2)()
            assert self.L.light_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, ptr(out), cnt) == 0
            return out, int(cnt[0]), int(cnt[1])
        out = self.cached(("frame",) + a.key, a.keep, make)
        return out if counters else out[0]
