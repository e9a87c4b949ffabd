"""Test-side helpers of the maximum-intensity projection tests: mip_render of tests/feature_ref.c (the MIP loop restated with the CPU
oracle's own statics) and tests/mip_bound_ref.c (the skip bound checked per sample), both loaded by tests/ref_library.py, and the small
volumes / transfer functions both tiers use."""
import ctypes as C

import numpy as np

from ref_library import Ref, SceneArgs, frame_array, ptr, volume_args


class MipRef(Ref):
    """mip_render of tests/feature_ref.c: (RGBA frame, per-pixel maximum) of a WHOLE frame; cached per (params, volume, tf)."""

    def __init__(self):
        super().__init__()
        self.L.mip_render.restype = C.c_int
        self.B.bound_check.restype = C.c_long

    def render(self, params, voxels, tf):
        a = SceneArgs(params, voxels, tf)

        def make():
            out, raw = frame_array(params, 4), frame_array(params, dtype=np.uint32)
            assert self.L.mip_render(*a.base, ptr(out), ptr(raw)) == 0
            return out, raw
        return self.cached(("mip",) + a.key, a.keep, make)

    def bound_violations(self, params, voxels):
        """(samples of the whole frame that exceed the kernel's TRILINEAR skip bound, smallest margin): tests/mip_bound_ref.c"""
        vox, volume = volume_args(voxels)
        margin = C.c_double()
        bad = self.B.bound_check(C.byref(params), *volume, C.byref(margin))
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
