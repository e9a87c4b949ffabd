"""Test-side helpers of the isosurface tests: iso_render of tests/feature_ref.c (vr_hip_render_iso restated with the CPU oracle's own
statics; tests/ref_library.py loads it), and the (volume, level) pairs both tiers use."""
import ctypes as C

import numpy as np

from ref_library import Ref, SceneArgs, frame_array, ptr, volume_args

# (volume, level in raw voxel units): what the GPU tier renders and the CPU tier checks the skipping emulation on
PAIRS = (("bucky", 100.0), ("blob_40x24x56", 100.0), ("blob_40x24x56", 200.0), ("shell48", 100.0), ("random_u16", 24.5 * 257), ("random_u16", 200.0 * 257),
         ("late_max", 24.5), ("late_max", 200.0), ("corner", 24.5), ("corner", 200.0), ("first_slice", 200.0), ("zeros", 24.5))
NO_SURFACE = (("corner", 200.0), ("zeros", 24.5))     # the level is never reached (corner: though the volume's maximum is 255)
GOLDEN_VOLUMES = ("bucky", "blob_40x24x56", "shell48")
VOLUMES = GOLDEN_VOLUMES + ("random_u16", "late_max", "corner", "zeros", "first_slice")      # the order tests/test_gpu_mip.py alternates the frame sizes by
SIZES = ((80, 80), (120, 72))                         # 72 rows: not a multiple of the 16-row workgroup tile


class IsoRef(Ref):
    """iso_render of tests/feature_ref.c: (RGBA frame, depth, {samples, fetches, hits}) of a WHOLE frame; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.L.iso_render.restype = C.c_int
        self.L.iso_dilated_maxima.restype = None

    def dilated_maxima(self, vox):
        """(32768 dilated block maxima, block edge) of the volume, built on the host"""
        def make():
            dil, bd = np.zeros(32768, np.uint8), C.c_uint32()
            self.L.iso_dilated_maxima(*volume_args(vox)[1], ptr(dil), C.byref(bd))
            return dil, int(bd.value)
        return self.cached(("dilated", vox.ctypes.data, vox.shape), vox, make)

    def render(self, params, voxels, tf, level, refine, skipping=False):
        """skipping: emulate the kernel's fetch skipping by the dilated block maxima (params.esl itself is not looked at)"""
        a = SceneArgs(params, voxels, tf)

        def make():
            out, depth, counters = frame_array(params, 4), frame_array(params, dtype=np.float32), (C.c_uint64 * 3)()
            dil, bd = self.dilated_maxima(a.keep[0]) if skipping else (None, 0)
            assert self.L.iso_render(*a.base, C.c_float(level), C.c_uint32(refine), ptr(dil), C.c_uint32(bd), ptr(out), ptr(depth), counters) == 0
            return out, depth, {"samples": int(counters[0]), "fetches": int(counters[1]), "hits": int(counters[2])}
        return self.cached(("iso",) + a.key + (float(np.float32(level)), int(refine), bool(skipping)), a.keep, make)


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
