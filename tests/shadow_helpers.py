"""Test-side helpers of the shadow tests: tests/shadow_ref.c (the light grid of include/vr_hip.h vr_hip_set_shadow and the composite frame
scaled by it, restated with the CPU oracle's own statics) compiled on demand into a temporary directory like tests/clip_ref.c, and the
lights, grids and scenes both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY, clip_floats
from mip_helpers import compile_test_library

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


class ShadowRef:
    """shadow_build / shadow_render of tests/shadow_ref.c; cached per argument set."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = ShadowRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="shadow_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "shadow_ref.c", "libshadow_ref.so")
        self.L.shadow_build.restype = C.c_int
        self.L.shadow_render.restype = C.c_int
        self._cache = {}

    def _cached(self, key, keep, make):
        if key not in self._cache:
            out = make()
            out.setflags(write=False)
            self._cache[key] = (out, keep)              # (keep: the arrays whose addresses are part of the key stay alive)
        return self._cache[key][0]

    def build(self, light, dims, step, voxels, tf, cutoff=CUTOFF, sampling=1, clip=None):
        """q as a (S, S, S) uint8 array indexed [z, y, x]; clip None = no clip set"""
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        z, y, x = vox.shape
        lf = np.array(light, np.float32)
        cf = None if clip is None else clip_floats(clip)

        def make():
            q = np.zeros((dims, dims, dims), np.uint8)
            rc = self.L.shadow_build(lf.ctypes.data_as(C.c_void_p), C.c_uint32(dims), C.c_float(step), C.c_float(cutoff), C.c_uint32(sampling),
                                     vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize), tf.ctypes.data_as(C.c_void_p),
                                     None if cf is None else cf.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p))
            assert rc == 0
            return q
        return self._cached(("q", lf.tobytes(), int(dims), float(np.float32(step)), float(np.float32(cutoff)), int(sampling), vox.ctypes.data, vox.shape,
                             tf.tobytes(), None if cf is None else cf.tobytes()), vox, make)

    def render(self, params, voxels, tf, esl, q=None, strength=1.0, clip=IDENTITY):
        """the composite frame (TRILINEAR modes) scaled by the light grid q (None: no shadow) under `clip`"""
        assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        esl = np.ascontiguousarray(esl, dtype=np.uint32)
        z, y, x = vox.shape
        cf = clip_floats(clip)
        qq = None if q is None else np.ascontiguousarray(q)

        def make():
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            rc = self.L.shadow_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize),
                                      tf.ctypes.data_as(C.c_void_p), esl.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p),
                                      None if qq is None else qq.ctypes.data_as(C.c_void_p), C.c_uint32(0 if qq is None else qq.shape[0]), C.c_float(strength),
                                      out.ctypes.data_as(C.c_void_p))
            assert rc == 0
            return out
        return self._cached(("frame", bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), esl.tobytes(), cf.tobytes(), None if qq is None else qq.tobytes(),
                             float(np.float32(strength))), vox, make)


def unlit(params):
    """the same frame with light_kd = 0: no diffuse term, the shadow factor alone"""
    p = params.copy()
    p.light_kd = 0.0
    return p
