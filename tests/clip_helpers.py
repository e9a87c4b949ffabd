"""Test-side helpers of the clip-region tests: tests/clip_ref.c (the three projections with the segment of every ray narrowed as
include/vr_hip.h vr_hip_set_clip defines it, restated with the CPU oracle's own statics) compiled on demand into a temporary directory
like tests/mip_ref.c, and the clip regions both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from mip_helpers import compile_test_library

# (box_min, box_max, plane): a missing box is the cube, a missing plane is zeros.  The box is the size at which every (volume, clip) of the
# GPU tier keeps 5 % of its pixels non-zero (tests/test_clip_model.py: the cap) — (-0.5, -0.25, -0.75) .. (0.25, 0.6, 0.5) left `corner`, whose
# isosurfaces are all but empty, at 4.2 % under BOTH
BOX = ((-0.6, -0.3, -0.8), (0.35, 0.65, 0.55), None)
PLANE = (None, None, (0.6, 0.3, -0.7416198, 0.1))
BOTH = (BOX[0], BOX[1], PLANE[2])
IDENTITY = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0))
NOTHING = (None, None, (0.0, 0.0, 1.0, -5.0))              # z >= 5: the kept half-space misses the cube
CLIPS = {"box": BOX, "plane": PLANE, "both": BOTH}


def parallel_plane(view):
    """PARALLEL: the plane through the centre whose normal is the screen-right axis of `view` — on an orthogonal view n . direction is
    exactly 0 where right_plane is exactly perpendicular to the direction in fp32, as it is for benchmark view 0"""
    r = np.array(list(view.right_plane), np.float64)
    n = r / np.sqrt((r ** 2).sum())
    return (None, None, (float(n[0]), float(n[1]), float(n[2]), 0.0))


def clip_floats(clip):
    """the ten floats of vr_clip"""
    box_min, box_max, plane = clip
    return np.array(list(box_min or (-1, -1, -1)) + list(box_max or (1, 1, 1)) + list(plane or (0, 0, 0, 0)), np.float32)


def set_clip(renderer, clip):
    renderer.set_clip(box_min=clip[0], box_max=clip[1], plane=clip[2])


class ClipRef:
    """clip_render / clip_mip_render / clip_iso_render of tests/clip_ref.c on WHOLE frames; cached per argument set."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = ClipRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="clip_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "clip_ref.c", "libclip_ref.so")
        for f in (self.L.clip_render, self.L.clip_mip_render, self.L.clip_iso_render):
            f.restype = C.c_int
        self._cache = {}

    @staticmethod
    def _inputs(params, voxels, tf, clip):
        assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        z, y, x = vox.shape
        return vox, tf, (C.c_uint32 * 3)(x, y, z), clip_floats(clip)

    def _cached(self, key, vox, make):
        if key not in self._cache:
            out = make()
            for a in out:
                a.setflags(write=False)
            self._cache[key] = (out, vox)               # (vox keeps the array whose address is part of the key alive)
        return self._cache[key][0]

    def composite(self, params, voxels, tf, esl, clip):
        vox, tf, dims, cf = self._inputs(params, voxels, tf, clip)
        esl = np.ascontiguousarray(esl, dtype=np.uint32)

        def make():
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            rc = self.L.clip_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), dims, C.c_uint32(vox.dtype.itemsize), tf.ctypes.data_as(C.c_void_p),
                                    esl.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
            assert rc == 0
            return (out,)
        return self._cached(("dvr", bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), esl.tobytes(), cf.tobytes()), vox, make)[0]

    def mip(self, params, voxels, tf, clip):
        vox, tf, dims, cf = self._inputs(params, voxels, tf, clip)

        def make():
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            rc = self.L.clip_mip_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), dims, C.c_uint32(vox.dtype.itemsize), tf.ctypes.data_as(C.c_void_p),
                                        cf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
            assert rc == 0
            return (out,)
        return self._cached(("mip", bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), cf.tobytes()), vox, make)[0]

    def iso(self, params, voxels, tf, level, refine, clip):
        """(RGBA frame, depth, rays): rays[..., :3] / rays[..., 3:] = origin / direction of every pixel's own ray"""
        vox, tf, dims, cf = self._inputs(params, voxels, tf, clip)

        def make():
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            depth = np.zeros((params.out_rows, params.out_width), np.float32)
            rays = np.zeros((params.out_rows, params.out_width, 6), np.float32)
            rc = self.L.clip_iso_render(C.byref(params), vox.ctypes.data_as(C.c_void_p), dims, C.c_uint32(vox.dtype.itemsize), tf.ctypes.data_as(C.c_void_p),
                                        C.c_float(level), C.c_uint32(refine), cf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                        depth.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p))
            assert rc == 0
            return out, depth, rays
        return self._cached(("iso", bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), float(np.float32(level)), int(refine), cf.tobytes()), vox, make)


def composite_params(vr, golden, oracle, name, vox, view, sampling, full_march):
    """Whole-frame composite parameters, lit: the default mode (esl on, the golden threshold) or the full march (esl off, threshold 1.0).
    Volumes without a golden state take the oracle's scene (default transfer function, their own ESL bits); returns (params, tf, esl)."""
    p = vr.VrParams()
    p.view = view
    if name in ("bucky", "blob_40x24x56", "shell48"):
        st = golden.volume_state(name)
        tf, esl, bd, bs, step, thr, kd = st["tf"], st["esl"], st["esl_block_dims"], st["esl_block_size"], st["ray_step"], st["ray_threshold"], st["light_kd"]
    else:
        tf, esl, bd, bs, step = scene_of(oracle, name, vox)
        thr, kd = 0.95, 0.7
    p.ray_step, p.light_kd = float(step), float(kd) if float(kd) > 0.01 else 0.7
    p.ray_threshold, p.esl = (1.0, 0) if full_march else (float(thr), 1)
    p.esl_block_dims = int(bd)
    for j in range(3):
        p.esl_block_size[j] = float(bs[j])
    p.sampling = sampling
    return vr.whole_frame(p), tf, esl


_scenes = {}


def scene_of(oracle, name, vox):
    if name not in _scenes:
        _scenes[name] = oracle.scene_for(vox)
    return _scenes[name]
