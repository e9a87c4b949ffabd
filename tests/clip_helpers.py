"""Test-side helpers of the clip-region tests: clip_render, clip_mip_render and clip_iso_render of tests/feature_ref.c (the three
projections with the segment of every ray narrowed as include/vr_hip.h vr_hip_set_clip defines it, restated with the CPU oracle's own
statics; tests/ref_library.py loads it), and the clip regions both tiers use."""
import ctypes as C

import numpy as np

from ref_library import Ref, SceneArgs, clip_floats, frame_array, ptr  # noqa: F401  (clip_floats: the tests take it from here)

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


def set_clip(renderer, clip):
    renderer.set_clip(box_min=clip[0], box_max=clip[1], plane=clip[2])


class ClipRef(Ref):
    """clip_render / clip_mip_render / clip_iso_render of tests/feature_ref.c on WHOLE frames; cached per argument set."""

    def __init__(self):
        super().__init__()
        for f in (self.L.clip_render, self.L.clip_mip_render, self.L.clip_iso_render):
            f.restype = C.c_int

    def composite(self, params, voxels, tf, esl, clip):
        a = SceneArgs(params, voxels, tf, esl, clip)

        def make():
            out = frame_array(params, 4)
            assert self.L.clip_render(*a.base, a.esl, a.clip, ptr(out)) == 0
            return (out,)
        return self.cached(("dvr",) + a.key, a.keep, make)[0]

    def mip(self, params, voxels, tf, clip):
        a = SceneArgs(params, voxels, tf, clip=clip)

        def make():
            out = frame_array(params, 4)
            assert self.L.clip_mip_render(*a.base, a.clip, ptr(out)) == 0
            return (out,)
        return self.cached(("mip",) + a.key, a.keep, make)[0]

    def iso(self, params, voxels, tf, level, refine, clip):
        """(RGBA frame, depth, rays): rays[..., :3] / rays[..., 3:] = origin / direction of every pixel's own ray"""
        a = SceneArgs(params, voxels, tf, clip=clip)

        def make():
            out, depth, rays = frame_array(params, 4), frame_array(params, dtype=np.float32), frame_array(params, 6, dtype=np.float32)
            assert self.L.clip_iso_render(*a.base, C.c_float(level), C.c_uint32(refine), a.clip, ptr(out), ptr(depth), ptr(rays)) == 0
            return out, depth, rays
        return self.cached(("iso",) + a.key + (float(np.float32(level)), int(refine)), a.keep, make)


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
