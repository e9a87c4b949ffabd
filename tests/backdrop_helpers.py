"""Test-side helpers of the backdrop tests: backdrop_render, hybrid_render and backdrop_segments of tests/feature_ref.c (the backdrop and
hybrid frames of include/vr_hip.h vr_hip_render_backdrop / vr_hip_render_hybrid, restated with the CPU oracle's own statics;
tests/ref_library.py loads it), the seeded generator of synthetic layers, and the isosurface levels both tiers use.  The volumes, views
and scenes of these tests are light_helpers.lit_volumes, light_helpers.lit_views and slab_helpers.slab_scene."""
import ctypes as C

import numpy as np

from clip_helpers import IDENTITY
from feature_random import generator
from light_helpers import LIT_VOLUMES, lit_views
from ref_library import Ref, SceneArgs, frame_array, ptr
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


class BackdropRef(Ref):
    """backdrop_render / hybrid_render / backdrop_segments of tests/feature_ref.c on WHOLE frames; cached per argument set."""

    def __init__(self):
        super().__init__()
        for f in (self.L.backdrop_render, self.L.hybrid_render, self.L.backdrop_segments):
            f.restype = C.c_int

    def render(self, params, voxels, tf, esl, rgba=None, depth=None, mode=POINT, clip=IDENTITY, lighting=None, q=None, strength=1.0, perturb=0):
        """the composite frame over the layer (rgba [rows, width, 4] uint8, depth [rows, width] float32; both None: the bytes of slab_render)"""
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength, mode)
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            assert rgba.shape == (params.out_rows, params.out_width, 4) and depth.shape == (params.out_rows, params.out_width)

        def make():
            out = frame_array(params, 4)
            assert self.L.backdrop_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, a.mode, C.c_uint32(perturb), ptr(rgba), ptr(depth), ptr(out)) == 0
            return (out,)
        key = ("backdrop",) + a.key + (None if rgba is None else rgba.tobytes(), None if depth is None else depth.tobytes(), int(perturb))
        return self.cached(key, a.keep, make)[0]

    def hybrid(self, params, voxels, tf, esl, level, refine, mode=POINT, clip=IDENTITY, lighting=None, q=None, strength=1.0, perturb=0):
        """(hybrid frame, depth, isosurface frame)"""
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength, mode)

        def make():
            out, dep, iso = frame_array(params, 4), frame_array(params, dtype=np.float32), frame_array(params, 4)
            assert self.L.hybrid_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, a.mode, C.c_uint32(perturb), C.c_float(level), C.c_uint32(refine),
                                        ptr(out), ptr(dep), ptr(iso)) == 0
            return out, dep, iso
        return self.cached(("hybrid",) + a.key + (float(np.float32(level)), int(refine), int(perturb)), a.keep, make)

    def segments(self, params, voxels, tf, esl, clip=IDENTITY):
        """[rows, width, 3] float32: kx, ky of the clipped segment and the k of the first sample of the accumulation loop; NaN = none"""
        a = SceneArgs(params, voxels, tf, esl, clip)

        def make():
            seg = frame_array(params, 3, dtype=np.float32)
            assert self.L.backdrop_segments(*a.base, a.esl, a.clip, ptr(seg)) == 0
            return (seg,)
        return self.cached(("segments",) + a.key, a.keep, make)[0]


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
    """slab_helpers.slab_scene in one of MARCHES"""
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, march != "default", step_factor)
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
    for v, (label, view) in enumerate(lit_views(vr, golden, name)):
        for m, march in enumerate(MARCHES):
            for factor in (1, 4):
                vox, p, tf, esl = march_scene(vr, golden, oracle, volumes, name, view, sampling, march, factor)
                rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=16 * v + 4 * m + factor)
                for params in (p, cue(p)):
                    yield (name, sampling, label, march, factor, params.light_kd), vox, params, tf, esl, rgba, depth
