"""Test-side helpers of the isosurface tests: tests/iso_ref.c (vr_hip_render_iso restated with the CPU oracle's own statics) compiled on
demand into a temporary directory like tests/mip_ref.c, and the (volume, level) pairs both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from mip_helpers import compile_test_library

# (volume, level in raw voxel units): what the GPU tier renders and the CPU tier checks the skipping emulation on
PAIRS = (("bucky", 100.0), ("blob_40x24x56", 100.0), ("blob_40x24x56", 200.0), ("shell48", 100.0), ("random_u16", 24.5 * 257), ("random_u16", 200.0 * 257),
         ("late_max", 24.5), ("late_max", 200.0), ("corner", 24.5), ("corner", 200.0), ("first_slice", 200.0), ("zeros", 24.5))
NO_SURFACE = (("corner", 200.0), ("zeros", 24.5))     # the level is never reached (corner: though the volume's maximum is 255)
GOLDEN_VOLUMES = ("bucky", "blob_40x24x56", "shell48")
VOLUMES = GOLDEN_VOLUMES + ("random_u16", "late_max", "corner", "zeros", "first_slice")      # the order tests/test_gpu_mip.py alternates the frame sizes by
SIZES = ((80, 80), (120, 72))                         # 72 rows: not a multiple of the 16-row workgroup tile


class IsoRef:
    """iso_render of tests/iso_ref.c: (RGBA frame, depth, {samples, fetches, hits}) of a WHOLE frame; cached per argument set."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = IsoRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="iso_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "iso_ref.c", "libiso_ref.so")
        self.L.iso_render.restype = C.c_int
        self.L.iso_dilated_maxima.restype = None
        self._cache = {}
        self._dilated = {}

    def dilated_maxima(self, vox):
        """(32768 dilated block maxima, block edge) of the volume, built on the host"""
        key = (vox.ctypes.data, vox.shape)
        if key not in self._dilated:
            z, y, x = vox.shape
            dil = np.zeros(32768, np.uint8)
            bd = C.c_uint32()
            self.L.iso_dilated_maxima(vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize), dil.ctypes.data_as(C.c_void_p), C.byref(bd))
            self._dilated[key] = (dil, int(bd.value), vox)
        return self._dilated[key][:2]

    def render(self, params, voxels, tf, level, refine, skipping=False):
        """skipping: emulate the kernel's fetch skipping by the dilated block maxima (params.esl itself is not looked at)"""
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        key = (bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), float(np.float32(level)), int(refine), bool(skipping))
        if key not in self._cache:
            assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
            z, y, x = vox.shape
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            depth = np.zeros((params.out_rows, params.out_width), np.float32)
            counters = (C.c_uint64 * 3)()
            dil, bd = self.dilated_maxima(vox) if skipping else (None, 0)
            rc = self.L.iso_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize),
                                   tf.ctypes.data_as(C.c_void_p), C.c_float(level), C.c_uint32(refine),
                                   dil.ctypes.data_as(C.c_void_p) if skipping else None, C.c_uint32(bd),
                                   out.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p), counters)
            assert rc == 0
            out.setflags(write=False)
            depth.setflags(write=False)
            self._cache[key] = (out, depth, {"samples": int(counters[0]), "fetches": int(counters[1]), "hits": int(counters[2])}, vox)
        return self._cache[key][:3]


def frame_params(vr, oracle, vox, view, sampling, esl, light_kd=0.7):
    """Whole-frame parameters.  What an isosurface frame must ignore is set to values that would show: the threshold, and an ESL block
    geometry that is NOT the volume's (the kernel takes the grid of the min/max scan)."""
    z, y, x = vox.shape
    p = vr.VrParams()
    p.view = view
    p.ray_step = float(oracle.default_ray_step((x, y, z)))
    p.ray_threshold, p.light_kd = 0.5, light_kd
    p.esl, p.esl_block_dims = esl, 3
    for j in range(3):
        p.esl_block_size[j] = 0.1
    p.sampling = sampling
    return vr.whole_frame(p)


def views_of(vr, golden, index):
    """The nine views of tests/test_gpu_mip.py: the eight benchmark views at 80 x 80 and 120 x 72, alternating with `index`, and golden
    case 32's far perspective view, most of whose rays miss."""
    out = [(f"view{i}", vr.benchmark_view(*SIZES[(i + index) % 2], i)) for i in range(8)]
    far = golden.params(next(c for c in golden.cases() if c["id"] == 32)).view
    return out + [("far_persp", far)]


def views_for(vr, golden, name):
    return views_of(vr, golden, VOLUMES.index(name))


def all_volumes(golden):
    from mip_helpers import synthetic_volumes
    v = {name: np.ascontiguousarray(golden.voxels(name)) for name in GOLDEN_VOLUMES}
    v.update(synthetic_volumes())
    return v


def depth_bits(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
