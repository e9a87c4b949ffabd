"""Test-side helpers of the maximum-intensity projection tests: tests/mip_ref.c (the MIP loop restated with the CPU oracle's own
statics) and tests/mip_bound_ref.c (the skip bound checked per sample) compiled on demand into a temporary directory, and the small
volumes / transfer functions both tiers use."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what oracle/Makefile builds libvr_oracle.so with
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-fopenmp"]


def compile_test_library(tmp_dir, source, name):
    lib = os.path.join(tmp_dir, name)
    subprocess.check_call(["gcc", *CFLAGS, "-o", lib, os.path.join(ROOT, "tests", source), "-lm"])
    return C.CDLL(lib)


class MipRef:
    """mip_render of tests/mip_ref.c: (RGBA frame, per-pixel maximum) of a WHOLE frame; cached per (params, volume, tf)."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = MipRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="mip_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "mip_ref.c", "libmip_ref.so")
        self.L.mip_render.restype = C.c_int
        self.B = compile_test_library(self.dir, "mip_bound_ref.c", "libmip_bound_ref.so")
        self.B.bound_check.restype = C.c_long
        self._cache = {}

    def render(self, params, voxels, tf):
        vox = np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        key = (bytes(params), vox.ctypes.data, vox.shape, tf.tobytes())
        if key not in self._cache:
            assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
            z, y, x = vox.shape
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            raw = np.zeros((params.out_rows, params.out_width), np.uint32)
            rc = self.L.mip_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize),
                                   tf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p))
            assert rc == 0
            out.setflags(write=False)
            raw.setflags(write=False)
            self._cache[key] = (out, raw, vox)          # (vox keeps the array whose address is part of the key alive)
        return self._cache[key][:2]

    def bound_violations(self, params, voxels):
        """(samples of the whole frame that exceed the kernel's TRILINEAR skip bound, smallest margin): tests/mip_bound_ref.c"""
        vox = np.ascontiguousarray(voxels)
        z, y, x = vox.shape
        margin = C.c_double()
        bad = self.B.bound_check(C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize), C.byref(margin))
        return int(bad), float(margin.value)


def ramp_tf():
    """A premultiplied transfer function without zero entries: every maximum, 0 included, gives a non-zero pixel, so a ray that
    hits the volume differs from one that misses, and neighbouring maxima differ in some channel."""
    i = np.arange(128, dtype=np.float32)
    a = (i + 1.0) / 128.0
    base = np.stack([i / 127.0, 1.0 - i / 127.0, np.abs(((i * 5.0) % 128.0) / 64.0 - 1.0), a], axis=1).astype(np.float32)
    tf = base.copy()
    tf[:, :3] *= base[:, 3:4]
    return tf


def random_u16():
    """56 x 24 x 40 voxels of 16 bits with independent low bytes"""
    return np.random.default_rng(5).integers(0, 65536, size=(40, 24, 56), dtype=np.uint16)


def synthetic_volumes():
    """name -> voxels (z, y, x) of the volumes the GPU tier adds to the golden ones"""
    rng = np.random.default_rng(11)
    late = np.zeros((64, 64, 64), np.uint8)                     # running maxima rise late: skipping has work to do
    late[:, :, 6:12] = rng.integers(20, 40, size=(64, 64, 6))   # a dim slab near one face
    late[:, :, 60:62] = rng.integers(180, 220, size=(64, 64, 2))   # one bright thin slab at the opposite face
    for z, y, x in ((9, 50, 30), (40, 13, 33), (33, 33, 20), (57, 8, 45)):
        late[z, y, x] = 250                                     # a few isolated bright voxels
    corner = np.zeros((32, 32, 32), np.uint8)
    corner[8, 8, 8] = 255                                       # on a block corner: a TRILINEAR bound without the one-voxel halo fails here
    first = rng.integers(0, 120, size=(32, 32, 32)).astype(np.uint8)
    first[0, :, :] = 200                                        # the first slice already holds the global maximum
    return {"random_u16": random_u16(), "late_max": late, "corner": corner, "zeros": np.zeros((32, 32, 32), np.uint8), "first_slice": first}


def lookup_index(raw, bytes_per_voxel, q8):
    """J(m): the upper index of the filtered transfer-function lookup of m, or the lower one when the (rounded) weight is 0"""
    scale = np.float32(128.0) / np.float32(255.0 if bytes_per_voxel == 1 else 65535.0)
    # fma(raw, scale, -0.5): the product of two floats and the sum with 0.5 are exact in double, so this is ONE rounding
    xb = (raw.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32)
    fl = np.floor(xb)
    a = xb - fl
    if q8:
        a = np.rint(a * np.float32(256)) / np.float32(256)
    i = fl.astype(np.int64)
    return np.where(a > 0, np.clip(i + 1, 0, 127), np.clip(i, 0, 127))
