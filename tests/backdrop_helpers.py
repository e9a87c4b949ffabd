"""Test-side helpers of the backdrop tests: tests/backdrop_ref.c (the backdrop and hybrid frames of include/vr_hip.h vr_hip_render_backdrop /
vr_hip_render_hybrid, restated with the CPU oracle's own statics) compiled on demand into a temporary directory like tests/slab_ref.c, the
seeded generator of synthetic layers, and the volumes, views and isosurface levels both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY, clip_floats
from feature_random import generator
from light_helpers import LIT_VOLUMES, lit_views, lit_volumes
from mip_helpers import compile_test_library
from slab_helpers import POINT, slab_scene

# what the GPU tier renders (with the eleven EDGE_SHAPES of tests/feature_random.py)
BACKDROP_VOLUMES = LIT_VOLUMES
# One isosurface level per volume of the GPU tier, chosen by hand, in raw voxel units: a surface INSIDE translucent matter.  The transfer
# functions are zero below 10 % density, so the levels lie well above that: the volume in front of the surface contributes, and the
# surface hides what lies behind it.  tests/test_backdrop_model.py holds the shares (surface pixels, pixels that differ from the
# isosurface frame, pixels that differ from the plain composite) to a fifth each and DESIGN.md section 4.11 lists what they are.
HYBRID_LEVELS = {"bucky": 110.5, "blob_40x24x56": 100.5, "random_u16": 130.5 * 257.0, "plateau": 120.5}
K_LT_D, NO_BLEND_AFTER_ERT, BYTE_OVER_255 = 1, 2, 3        # the `perturb` of backdrop_render: the sensitivity test's wrong readings
STREAM = 411                                              # the generator stream of the synthetic layers (feature_random.generator)


def backdrop_volumes(golden):
    return lit_volumes(golden)


def backdrop_views(vr, golden, name):
    return lit_views(vr, golden, name)


def backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march, step_factor=1):
    """(voxels, params, tf, esl) of a volume's composite frame: slab_helpers.slab_scene"""
    return slab_scene(vr, golden, oracle, volumes, name, view, sampling, full_march, step_factor)


class BackdropRef:
    """backdrop_render / hybrid_render / backdrop_segments of tests/backdrop_ref.c on WHOLE frames; cached per argument set."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = BackdropRef()
        return cls._inst

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="backdrop_ref_")
        atexit.register(shutil.rmtree, self.dir, ignore_errors=True)
        self.L = compile_test_library(self.dir, "backdrop_ref.c", "libbackdrop_ref.so")
        for f in (self.L.backdrop_render, self.L.hybrid_render, self.L.backdrop_segments):
            f.restype = C.c_int
        self._cache = {}

    @staticmethod
    def _scene_args(params, voxels, tf, esl, clip, lighting, q, strength, mode):
        assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
        vox = voxels if voxels.flags["C_CONTIGUOUS"] else np.ascontiguousarray(voxels)
        tf = np.ascontiguousarray(tf, dtype=np.float32)
        esl = np.ascontiguousarray(esl, dtype=np.uint32)
        z, y, x = vox.shape
        cf = clip_floats(clip)
        lf = None if lighting is None else np.array(lighting[:3], np.float32)
        shin = 0 if lighting is None else int(lighting[3])
        qq = None if q is None else np.ascontiguousarray(q)
        key = (bytes(params), vox.ctypes.data, vox.shape, tf.tobytes(), esl.tobytes(), cf.tobytes(), None if lf is None else lf.tobytes(), shin,
               None if qq is None else qq.tobytes(), float(np.float32(strength)), int(mode))
        args = [C.byref(params), vox.ctypes.data_as(C.c_void_p), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize),
                tf.ctypes.data_as(C.c_void_p), esl.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p),
                None if lf is None else lf.ctypes.data_as(C.c_void_p), C.c_uint32(shin),
                None if qq is None else qq.ctypes.data_as(C.c_void_p), C.c_uint32(0 if qq is None else qq.shape[0]),
                C.c_float(strength), C.c_uint32(mode)]
        return key, args, (vox, tf, esl, cf, lf, qq)

    def render(self, params, voxels, tf, esl, rgba=None, depth=None, mode=POINT, clip=IDENTITY, lighting=None, q=None, strength=1.0, perturb=0):
        """the composite frame over the layer (rgba [rows, width, 4] uint8, depth [rows, width] float32; both None: the bytes of slab_render)"""
        key, args, keep = self._scene_args(params, voxels, tf, esl, clip, lighting, q, strength, mode)
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            assert rgba.shape == (params.out_rows, params.out_width, 4) and depth.shape == (params.out_rows, params.out_width)
        key = ("backdrop",) + key + (None if rgba is None else rgba.tobytes(), None if depth is None else depth.tobytes(), int(perturb))
        if key not in self._cache:
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            rc = self.L.backdrop_render(*args, C.c_uint32(perturb), None if rgba is None else rgba.ctypes.data_as(C.c_void_p),
                                        None if depth is None else depth.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
            assert rc == 0
            out.setflags(write=False)
            self._cache[key] = (out, keep)
        return self._cache[key][0]

    def hybrid(self, params, voxels, tf, esl, level, refine, mode=POINT, clip=IDENTITY, lighting=None, q=None, strength=1.0, perturb=0):
        """(hybrid frame, depth, isosurface frame)"""
        key, args, keep = self._scene_args(params, voxels, tf, esl, clip, lighting, q, strength, mode)
        key = ("hybrid",) + key + (float(np.float32(level)), int(refine), int(perturb))
        if key not in self._cache:
            out = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            iso = np.zeros((params.out_rows, params.out_width, 4), np.uint8)
            dep = np.zeros((params.out_rows, params.out_width), np.float32)
            rc = self.L.hybrid_render(*args, C.c_uint32(perturb), C.c_float(level), C.c_uint32(refine), out.ctypes.data_as(C.c_void_p),
                                      dep.ctypes.data_as(C.c_void_p), iso.ctypes.data_as(C.c_void_p))
            assert rc == 0
            for a in (out, dep, iso):
                a.setflags(write=False)
            self._cache[key] = ((out, dep, iso), keep)
        return self._cache[key][0]

    def segments(self, params, voxels, tf, esl, clip=IDENTITY):
        """[rows, width, 3] float32: kx, ky of the clipped segment and the k of the first sample of the accumulation loop; NaN = none"""
        key, args, keep = self._scene_args(params, voxels, tf, esl, clip, None, None, 1.0, 0)
        key = ("segments",) + key
        if key not in self._cache:
            seg = np.zeros((params.out_rows, params.out_width, 3), np.float32)
            rc = self.L.backdrop_segments(*args[:7], seg.ctypes.data_as(C.c_void_p))
            assert rc == 0
            seg.setflags(write=False)
            self._cache[key] = (seg, keep)
        return self._cache[key][0]


def sample_ks(k0, step, n):
    """k of sample n of a march that starts at k0, accumulated as the march accumulates it: n float32 additions of the step"""
    k = np.array(k0, np.float32, copy=True)
    step = np.float32(step)
    left = np.array(n, np.int64, copy=True)
    while (left > 0).any():
        k = np.where(left > 0, (k + step).astype(np.float32), k)
        left = left - 1
    return k


def synthetic_layer(ref, params, voxels, tf, esl, clip=IDENTITY, salt=0, all_bytes=False):
    """(rgba, depth) of a seeded synthetic layer for a whole frame.  Colour bytes are random (all_bytes: every byte value in every channel,
    frames of at least 256 pixels).  Depths are a per-pixel mix of: -1, NaN, 0, +inf, a value before kx, inside [kx, ky], beyond ky, and
    exactly on a sample k0 + n * step accumulated as the march accumulates it (pixels without a segment or a first sample take a plain
    positive value there)."""
    rng = generator(STREAM + 1000 * salt)
    rows, width = params.out_rows, params.out_width
    rgba = rng.integers(0, 256, size=(rows, width, 4), dtype=np.uint8)
    if all_bytes:
        assert rows * width >= 256
        flat = rgba.reshape(-1, 4)
        for ch in range(4):
            flat[rng.permutation(rows * width)[:256], ch] = np.arange(256, dtype=np.uint8)
    seg = ref.segments(params, voxels, tf, esl, clip)
    kx, ky, k0 = seg[..., 0], seg[..., 1], seg[..., 2]
    kind = rng.integers(0, 8, size=(rows, width))
    u = rng.random(size=(rows, width)).astype(np.float32)
    have = ~np.isnan(kx)
    span = np.where(have, ky - kx, np.float32(1.0)).astype(np.float32)
    base = np.where(have, kx, np.float32(1.0)).astype(np.float32)
    step = np.float32(params.ray_step)
    nmax = np.where(~np.isnan(k0), np.floor((ky - k0) / step), 0.0)
    n = np.floor(u * (np.nan_to_num(nmax) + 1.0)).astype(np.int64)
    on_sample = sample_ks(np.where(np.isnan(k0), base, k0), step, np.minimum(n, 4096))
    depth = np.select(
        [kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6],
        [np.float32(-1.0), np.float32(np.nan), np.float32(0.0), np.float32(np.inf), np.maximum(base * u, np.float32(0.0)).astype(np.float32),
         (base + span * u).astype(np.float32), (base + span * (np.float32(1.0) + u)).astype(np.float32)],
        on_sample).astype(np.float32)
    rgba.setflags(write=False)
    depth.setflags(write=False)
    return rgba, depth


MARCHES = ("default", "full", "ert")     # esl on + the golden threshold; esl off + threshold 1; esl off + threshold 0.95 (early termination alone)


def march_scene(vr, golden, oracle, volumes, name, view, sampling, march, step_factor=1):
    """backdrop_scene in one of MARCHES"""
    vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, march != "default", step_factor)
    if march == "ert":
        p = p.copy()
        p.ray_threshold = 0.95
    return vox, p, tf, esl


def tier_frames(vr, golden, oracle, volumes, name, sampling):
    """The frames of the GPU tier's main test for one (volume, sampling), each with its synthetic layer: nine views x MARCHES x {the ray step,
    four times it: the clamping variant} x {cue-lit, light_kd = 0}.  Yields (what, voxels, params, tf, esl, rgba, depth); the CPU tier
    walks the same list."""
    from light_helpers import cue
    ref = BackdropRef.instance()
    for v, (label, view) in enumerate(backdrop_views(vr, golden, name)):
        for m, march in enumerate(MARCHES):
            for factor in (1, 4):
                vox, p, tf, esl = march_scene(vr, golden, oracle, volumes, name, view, sampling, march, factor)
                rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=16 * v + 4 * m + factor)
                for params in (p, cue(p)):
                    yield (name, sampling, label, march, factor, params.light_kd), vox, params, tf, esl, rgba, depth
