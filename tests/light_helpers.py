"""Test-side helpers of the lighting tests: tests/light_ref.c (the gradient-lit composite frame of include/vr_hip.h vr_hip_set_lighting,
restated with the CPU oracle's own statics) compiled on demand into a temporary directory like tests/shadow_ref.c, and the lightings,
volumes and views both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY, clip_floats
from iso_helpers import all_volumes, views_of
from mip_helpers import compile_test_library

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


class LightRef:
    """light_render of tests/light_ref.c; cached per argument set."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = LightRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="light_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "light_ref.c", "liblight_ref.so")
        self.L.light_render.restype = C.c_int
        self._cache = {}

    def render(self, params, voxels, tf, esl, lighting, q=None, strength=1.0, clip=IDENTITY, counters=False):
        """the composite frame (TRILINEAR modes) lit by `lighting` = (ambient, diffuse, specular, shininess_log2), scaled by the light grid q
        (None: no shadow) under `clip`; counters=True: (frame, dense samples, dense samples with a zero gradient)"""
        assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        esl = np.ascontiguousarray(esl, dtype=np.uint32)
        z, y, x = vox.shape
        cf = clip_floats(clip)
        lf = np.array(lighting[:3], np.float32)
        qq = None if q is None else np.ascontiguousarray(q)
        key = ("frame", bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), esl.tobytes(), cf.tobytes(), lf.tobytes(), int(lighting[3]),
               None if qq is None else qq.tobytes(), float(np.float32(strength)))
        if key not in self._cache:
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            cnt = (C.c_uint64 * 2)()
            rc = self.L.light_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize),
                                     tf.ctypes.data_as(C.c_void_p), esl.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p),
                                     C.c_uint32(int(lighting[3])), None if qq is None else qq.ctypes.data_as(C.c_void_p),
                                     C.c_uint32(0 if qq is None else qq.shape[0]), C.c_float(strength), out.ctypes.data_as(C.c_void_p), cnt)
            assert rc == 0
            out.setflags(write=False)
            self._cache[key] = (out, int(cnt[0]), int(cnt[1]), vox)       # (vox: the array whose address is part of the key stays alive)
        out, dense, flat, _ = self._cache[key]
        return (out, dense, flat) if counters else out
