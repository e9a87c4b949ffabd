"""Generators shared by tests/test_feature_random_model.py (CPU) and tests/test_gpu_feature_random.py (GPU): random and ragged inputs for
the MIP, the isosurface, the clip region, the light grid with its shadowed frames and the gradient lighting.  The volumes and views are
those of tests/test_gpu_random.py (odd extents, one extent forced to 1 / 2 / 8 / 16 / 33, cameras inside the cube, exact zeros in the
direction, the four-fold ray step); this module adds a clip, a light, a grid size, a lighting and an isosurface level per frame, and the
hand-made EDGE_SHAPES.  Everything is drawn from numpy generators seeded from VR_TEST_SEED (default 20261019), one per list of frames, so
that both tiers see the same frames whatever the order of the tests.  The slab, backdrop and hybrid frames (ExpectedLayers) reuse those
frames as they are — nothing more is drawn from the scene generators — and take their depth layers from backdrop_helpers.synthetic_layer
under salts of 2000 and above.  The depth frames and picks (ExpectedDepth, depth_draws) reuse them too: their opacities follow from
the frames' indices, and the pixels of the picks and the partitions come from a stream of their own.  A plain module: no fixtures."""
import os

import numpy as np

from clip_helpers import BOTH, IDENTITY
from light_helpers import PHONG
from shadow_helpers import LIGHTS
from test_gpu_random import random_params, random_scene

SEED = int(os.environ.get("VR_TEST_SEED", "20261019"))
# No generated ray step is below this: a ray through the cube (length <= 2 sqrt 3 < 4) has at most 4 * 64 samples.  The default step of a
# 1 x 1 x 1 volume is 0, with which a CPU march never advances; the library refuses steps below 1e-6, the restatements do not.
MIN_STEP = 1.0 / 64.0
SHADOW_DIMS = (2, 3, 5, 9, 17)
SCENES, FRAMES_PER_SCENE = 14, 4
WIDE = (0, 1, 2, 4)                                  # vr_hip_set_wide_addressing, alternated per scene

# (x, y, z): the smallest shapes that put a gradient fetch, a partial brick (edge 8), a partial block and a one-voxel-thick axis under
# every kernel.  1 x 1 x 1 is not among them: its default ray step is 0 (MIN_STEP above).
EDGE_SHAPES = ((2, 2, 2), (1, 9, 17), (9, 1, 7), (7, 9, 1), (8, 8, 8), (9, 9, 9), (33, 8, 16), (65, 3, 5), (3, 5, 65), (17, 31, 2), (1, 1, 40))
EDGE_DTYPES = ("uint8", "uint16")
EDGE_VIEWS = (0, 1, 5)                               # benchmark views: along an axis, oblique orthogonal, perspective
EDGE_SIZE = (48, 40)
EDGE_CLIPS = (("both", BOTH), ("identity", IDENTITY))
EDGE_LIGHT, EDGE_S, EDGE_LIGHTING, EDGE_REFINE = LIGHTS["inside"], 5, PHONG, 4


def generator(stream):
    """the numpy generator of one list of frames: seeded from VR_TEST_SEED and the list's number"""
    return np.random.default_rng([SEED, stream])


def _f32(v):
    return float(np.float32(v))


def clamp_step(step):
    return _f32(max(_f32(step), MIN_STEP))


def random_clip(rng):
    """(box_min, box_max, plane) as clip_helpers has them: a box only, a plane only, or both.  The box corners lie in [-1, 1] and every edge
    is at least 0.5 long; with probability 0.25 one face lies exactly on the cube's.  With probability 0.25 the plane's normal is an exact
    axis unit vector: an axis-aligned view along another axis is then exactly parallel to it (n . d == 0 with exact zeros)."""
    kind = int(rng.integers(0, 3))
    box_min = box_max = plane = None
    if kind != 1:
        lo = [_f32(rng.uniform(-1.0, 0.1)) for _ in range(3)]
        hi = [_f32(min(1.0, lo[j] + rng.uniform(0.5, 1.9))) for j in range(3)]
        if rng.random() < 0.25:
            axis = int(rng.integers(0, 3))
            if rng.random() < 0.5:
                lo[axis] = -1.0
            else:
                hi[axis] = 1.0
        box_min, box_max = tuple(lo), tuple(hi)
    if kind != 0:
        if rng.random() < 0.25:
            n = np.zeros(3, np.float32)
            n[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
        else:
            n = rng.normal(size=3).astype(np.float32)
            n /= np.linalg.norm(n)
        plane = (float(n[0]), float(n[1]), float(n[2]), _f32(rng.uniform(-0.3, 0.7)))      # d > 0 keeps the centre
    return box_min, box_max, plane


def random_light(rng, dims):
    """a normal draw of scale 1.5 (mostly outside), a point inside the cube, exactly a node -1 + 2 i / (dims - 1) of the light grid, or a
    point on a face of the cube"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return tuple(_f32(v) for v in rng.normal(scale=1.5, size=3))
    if kind == 1:
        return tuple(_f32(v) for v in rng.uniform(-0.9, 0.9, size=3))
    if kind == 2:
        return tuple(_f32(np.float32(-1.0) + np.float32(2.0) * np.float32(int(rng.integers(0, dims))) / np.float32(dims - 1)) for _ in range(3))
    pos = [_f32(v) for v in rng.uniform(-1.0, 1.0, size=3)]
    pos[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
    return tuple(pos)


def random_lighting(rng):
    """(ambient, diffuse, specular, shininess_log2): coefficients in [0, 1], each exactly 0 or 1 with probability 0.15; 0..10"""
    k = []
    for _ in range(3):
        v = _f32(rng.random())
        if rng.random() < 0.15:
            v = float(rng.integers(0, 2))
        k.append(v)
    return k[0], k[1], k[2], int(rng.integers(0, 11))


def random_level(rng, vox, tf=None):
    """A quantile between 0.3 and 0.9 of the volume's non-zero values, plus 0.5 (raw voxel units): most isosurfaces are not empty.  With a
    transfer function, up to eight quantiles are drawn until the surface's colour — the filtered lookup of the level — has some alpha: a
    random transfer function has holes, and a surface looked up in one is black whatever its shading does."""
    nz = vox[vox > 0]
    if not nz.size:
        return 0.5
    for _ in range(8):
        level = float(np.floor(np.quantile(nz, float(rng.uniform(0.3, 0.9))))) + 0.5
        if tf is None:
            break
        x = np.float32(level) * (np.float32(128.0) / np.float32(255.0 if vox.dtype == np.uint8 else 65535.0)) - np.float32(0.5)
        i = int(np.floor(x))
        if max(np.asarray(tf, np.float32).reshape(128, 4)[min(max(j, 0), 127), 3] for j in (i, i + 1)) > 0.02:
            break
    return level


def with_sampling(params, sampling, esl=None):
    p = params.copy()
    p.sampling = sampling
    if esl is not None:
        p.esl = esl
    return p


class Frame:
    """What one frame of the feature tests renders: `p` the composite's parameters (TRILINEAR or Q8), `mip` / `iso` the parameters of the two
    projections without fetch skipping (the GPU tier also renders them with esl = 1), the clip, the shadow (light, S, builder step and
    sampling, strength), the lighting, the isosurface (level, refine) and the order in which the GPU tier clears the three states."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def camera_inside(self):
        return all(abs(self.p.view.origin[j]) < 1.0 for j in range(3))

    def axis_aligned(self):
        return sorted(abs(self.p.view.direction[j]) for j in range(3)) == [0.0, 0.0, 1.0]


class Scene:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def describe(self):
        return f"{self.name} dims {self.vox.shape[::-1]} {self.vox.dtype}"


def random_frame(rng, vr, scene):
    S = int(rng.choice(SHADOW_DIMS))
    p = random_params(rng, vr, scene.bd, scene.bs, scene.ray_step, int(rng.choice([vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8])))
    p.ray_step = clamp_step(p.ray_step)
    return Frame(p=p, mip=with_sampling(p, int(rng.choice([vr.SAMPLE_NEAREST, vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8])), 0),
                 iso=with_sampling(p, int(rng.choice([vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8])), 0),
                 clip=random_clip(rng), S=S, light=random_light(rng, S), shadow_step=clamp_step(np.float32(scene.ray_step) * np.float32(rng.uniform(0.5, 1.5))),
                 shadow_sampling=int(rng.choice([vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8])), strength=_f32(rng.choice([1.0, 1.0, rng.uniform(0.2, 1.0)])),
                 lighting=random_lighting(rng), level=random_level(rng, scene.vox, scene.tf), refine=int(rng.integers(0, 9)),
                 clear_order=[int(i) for i in rng.permutation(3)])


_lists = {}


def random_scenes(oracle, vr, stream=0, scenes=SCENES, frames=FRAMES_PER_SCENE):
    """`scenes` random volumes with `frames` frames each, the same objects on every call (the restatements cache by the arrays' addresses)"""
    key = (stream, scenes, frames)
    if key not in _lists:
        rng = generator(stream)
        out = []
        for i in range(scenes):
            vox, tf, esl, bd, bs, ray_step = random_scene(rng, oracle, vr)
            vox = np.ascontiguousarray(vox)
            vox.setflags(write=False)
            s = Scene(name=f"scene {i}", vox=vox, tf=tf, esl=esl, bd=bd, bs=bs, ray_step=ray_step,
                      layout=vr.LAYOUT_BRICKED if i % 3 else vr.LAYOUT_LINEAR, wide=WIDE[i % len(WIDE)])
            s.frames = [random_frame(rng, vr, s) for _ in range(frames)]
            out.append(s)
        _lists[key] = out
    return _lists[key]


HOLED_STREAM, HOLED_SCENES, HOLED_FRAMES = 7, 6, 4


def holed_scenes(oracle, vr):
    """Scenes for the pre-integration's skipped samples, from a generator stream of their own (the frames of random_scenes stay what they
    are).  The random volumes are smooth: between two consecutive samples the value hardly ever jumps from what a wave may skip — below the
    largest power of two inside the transfer function's leading zeros — to what shows, so a sample behind a skipped one contributes
    nothing there.  Here a slab of exact zeros, a third to a half of the volume thick, is cut through a random volume of 12 to 39
    voxels per axis, and the random transfer function has at least its first entry zero: whole waves skip inside the slab, and the
    first sample behind it needs the coordinate of a skipped predecessor.  Frames are redrawn until they are 16 pixels or more a side."""
    key = ("holed",)
    if key not in _lists:
        rng = generator(HOLED_STREAM)
        out = []
        while len(out) < HOLED_SCENES:
            vox = random_scene(rng, oracle, vr)[0]
            if min(vox.shape) < 12:
                continue
            vox = np.array(vox)
            axis = int(rng.integers(0, 3))
            n = vox.shape[axis]
            thick = int(rng.integers(n // 3, n // 2 + 1))
            lo = int(rng.integers(2, n - thick - 1))
            cut = [slice(None)] * 3
            cut[axis] = slice(lo, lo + thick)
            vox[tuple(cut)] = 0
            vox = np.ascontiguousarray(vox)
            vox.setflags(write=False)
            base = rng.random((128, 4)).astype(np.float32)
            base[:, 3] *= (rng.random(128) < 0.7)
            base[: int(rng.integers(1, 40)), 3] = 0
            tf, esl, bd, bs, ray_step = oracle.scene_for(vox, base)
            i = len(out)
            s = Scene(name=f"holed scene {i}", vox=vox, tf=tf, esl=esl, bd=bd, bs=bs, ray_step=ray_step,
                      layout=vr.LAYOUT_BRICKED if i % 2 else vr.LAYOUT_LINEAR, wide=WIDE[i % len(WIDE)])
            s.frames = []
            while len(s.frames) < HOLED_FRAMES:
                f = random_frame(rng, vr, s)
                if min(f.p.view.width, f.p.view.height) >= 16:       # two waves a side at the least: it is whole waves that skip
                    s.frames.append(f)
            out.append(s)
        _lists[key] = out
    return _lists[key]


def edge_volume(shape_xyz, dtype):
    """a deterministic field that is nowhere constant: non-zero gradients and values either side of 128 on every shape of EDGE_SHAPES"""
    x, y, z = shape_xyz
    zz, yy, xx = np.mgrid[0:z, 0:y, 0:x]
    v = ((37 * xx + 59 * yy + 83 * zz + 90) % 256).astype(np.uint8)
    if np.dtype(dtype) == np.uint16:
        v = v.astype(np.uint16) * 257
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


_edges = {}


def edge_scene(oracle, vr, shape_xyz, dtype):
    """The Scene of one edge shape: the default transfer function, three views at 48 x 40 (default mode TRILINEAR, full march Q8, default
    mode TRILINEAR), one Frame per (view, clip of EDGE_CLIPS)"""
    key = (tuple(shape_xyz), str(np.dtype(dtype)))
    if key not in _edges:
        vox = edge_volume(shape_xyz, dtype)
        tf, esl, bd, bs, ray_step = oracle.scene_for(vox)
        step = clamp_step(ray_step)
        s = Scene(name="edge", vox=vox, tf=tf, esl=esl, bd=bd, bs=bs, ray_step=step, frames=[])
        level = 128.0 * (257.0 if vox.dtype == np.uint16 else 1.0)
        for n, index in enumerate(EDGE_VIEWS):
            p = vr.VrParams()
            p.view = vr.benchmark_view(*EDGE_SIZE, index)
            p.ray_step, p.light_kd = step, 0.7
            p.ray_threshold, p.esl = (1.0, 0) if n == 1 else (0.95, 1)
            p.esl_block_dims = int(bd)
            for j in range(3):
                p.esl_block_size[j] = float(bs[j])
            p.sampling = vr.SAMPLE_TRILINEAR_Q8 if n == 1 else vr.SAMPLE_TRILINEAR
            vr.whole_frame(p)
            for clip_name, clip in EDGE_CLIPS:
                s.frames.append(Frame(p=p, mip=with_sampling(p, (vr.SAMPLE_TRILINEAR, vr.SAMPLE_NEAREST, vr.SAMPLE_TRILINEAR_Q8)[n], 0),
                                      iso=with_sampling(p, p.sampling, 0), clip=clip, clip_name=clip_name, view=index, S=EDGE_S, light=EDGE_LIGHT,
                                      shadow_step=step, shadow_sampling=p.sampling, strength=1.0, lighting=EDGE_LIGHTING, level=level, refine=EDGE_REFINE,
                                      clear_order=[0, 1, 2]))
        _edges[key] = s
    return _edges[key]


class Expected:
    """The restatements' answers for one (scene, frame): what the GPU tier compares with and the CPU tier holds the caps on"""

    def __init__(self, scene, f):
        from clip_helpers import ClipRef
        from light_helpers import LightRef
        from shadow_helpers import CUTOFF, ShadowRef
        v, tf, esl = scene.vox, scene.tf, scene.esl
        clip_ref, shadow_ref, light_ref = ClipRef.instance(), ShadowRef.instance(), LightRef.instance()
        self.composite = clip_ref.composite(f.p, v, tf, esl, f.clip)
        self.mip = clip_ref.mip(f.mip, v, tf, f.clip)
        self.iso, self.depth, _ = clip_ref.iso(f.iso, v, tf, f.level, f.refine, f.clip)
        self.q = shadow_ref.build(f.light, f.S, f.shadow_step, v, tf, CUTOFF, f.shadow_sampling, clip=f.clip)
        self.shadowed = shadow_ref.render(f.p, v, tf, esl, self.q, f.strength, f.clip)
        self.lit, self.dense, self.flat = light_ref.render(f.p, v, tf, esl, f.lighting, self.q, f.strength, clip=f.clip, counters=True)


def layer_salt(scene_index, frame_index):
    """the salt of a random frame's synthetic layer (backdrop_helpers.synthetic_layer); the tests of the two feature files stay below 1000"""
    return 2000 + 8 * scene_index + frame_index


EDGE_SALT = 3000                                     # the layers of the edge shapes: EDGE_SALT + 8 * (2 * shape + dtype) + frame


class ExpectedLayers:
    """The restatements' answers for the slab, backdrop and hybrid frames of one (scene, frame), beside Expected so that the tests of the
    older features do not pay for them: slab_render, backdrop_render and hybrid_render under the frame's clip, point classified with the cue
    and — `*_all` — slab classified under the frame's lighting, light grid and strength.  The synthetic layer comes from
    backdrop_helpers.synthetic_layer, which has its own generator stream: the frames draw nothing for it."""

    def __init__(self, scene, f, salt=None):
        """salt None: the hybrid frames alone (they take no layer)"""
        from backdrop_helpers import BackdropRef, synthetic_layer
        from shadow_helpers import CUTOFF, ShadowRef
        from slab_helpers import POINT, SLAB, SlabRef
        v, tf, esl = scene.vox, scene.tf, scene.esl
        slab_ref, ref = SlabRef.instance(), BackdropRef.instance()
        self.q = ShadowRef.instance().build(f.light, f.S, f.shadow_step, v, tf, CUTOFF, f.shadow_sampling, clip=f.clip)
        states = (SLAB, f.clip, f.lighting, self.q, f.strength)
        self.hybrid, self.hybrid_depth, self.hybrid_iso = ref.hybrid(f.p, v, tf, esl, f.level, f.refine, POINT, f.clip)
        self.hybrid_all = ref.hybrid(f.p, v, tf, esl, f.level, f.refine, *states)[0]
        if salt is None:
            return
        self.slab, self.samples, self.wide, self.narrow = slab_ref.render(f.p, v, tf, esl, SLAB, f.clip, counters=True)
        self.slab_all = slab_ref.render(f.p, v, tf, esl, *states)
        self.rgba, self.depth = synthetic_layer(ref, f.p, v, tf, esl, f.clip, salt=salt)
        self.backdrop = ref.render(f.p, v, tf, esl, self.rgba, self.depth, POINT, f.clip)
        self.backdrop_all = ref.render(f.p, v, tf, esl, self.rgba, self.depth, *states)


# ---- the depth frames and picks on the same lists (tests/test_depth_random_model.py, tests/test_gpu_depth_random.py) ----
# Nothing here draws from the streams of the lists above: the opacity of a frame follows from its indices, and the pixels of the picks and
# the partitions come from DEPTH_STREAM, which no other list uses (0-7, 99, 411 + 1000 * salt, 412 and 611 are taken).

DEPTH_STREAM = 8
DEPTH_OPACITIES = (0.1, 0.5, 0.9)
DEPTH_MODES = ("first", "peak", "mean")              # depth_helpers.MODES
PICK_MAX, PICK_DRAWN = 256, 60                       # vr_hip_pick takes 256 pixels a call; the larger frames: four corners and 60 drawn pixels
THRESHOLD, ABOVE_THRESHOLD = "threshold", "above"
# FIRST at the edges of (0, 1]: the smallest subnormal, the smallest normal, 1, and — on the frames that terminate early — the frame's
# ray_threshold and the next float32 above it
EDGE_OPACITIES = (float(np.float32(1e-45)), float(np.finfo(np.float32).tiny), 1.0, THRESHOLD, ABOVE_THRESHOLD)


def depth_opacity(scene_index, frame_index):
    return DEPTH_OPACITIES[(scene_index + frame_index) % 3]


def edge_opacities(p):
    """EDGE_OPACITIES for the frame `p` as (label, float32 value) pairs: the last two only where ray_threshold < 1"""
    t = np.float32(p.ray_threshold)
    out = [("subnormal", EDGE_OPACITIES[0]), ("tiny", EDGE_OPACITIES[1]), ("one", EDGE_OPACITIES[2])]
    if t < np.float32(1.0):
        out += [(THRESHOLD, float(t)), (ABOVE_THRESHOLD, float(np.nextafter(t, np.float32(2.0))))]
    return out


def full_march(p):
    """a copy of the params without leaping and early termination: the march itself meets whatever the volume holds"""
    q = p.copy()
    q.esl, q.ray_threshold = 0, 1.0
    return q


def depth_list(oracle, vr, which):
    """[(n, scene index, frame index, scene, frame, opacity)] of the "random" (56) or "holed" (24) frames, n counting the frames"""
    scenes = random_scenes(oracle, vr) if which == "random" else holed_scenes(oracle, vr)
    return [(s * len(scene.frames) + i, s, i, scene, f, depth_opacity(s, i)) for s, scene in enumerate(scenes) for i, f in enumerate(scene.frames)]


class ExpectedDepth:
    """depth_render's answers for one (scene, frame) under the frame's clip, beside Expected and ExpectedLayers: what the GPU tier compares
    with and the CPU tier holds the caps on.  `p`: other params for the same view (full_march); the frames are the restatement's cached ones."""

    def __init__(self, scene, f, opacity, p=None):
        from depth_helpers import DepthRef
        self.ref, self.scene, self.f, self.p, self.opacity = DepthRef.instance(), scene, f, (f.p if p is None else p), opacity

    def frame(self, cmode, mode, opacity=None, perturb=0):
        s = self.scene
        return self.ref.render(self.p, s.vox, s.tf, s.esl, self.opacity if opacity is None else opacity, mode, cmode, self.f.clip, perturb)


def pick_state(n):
    """(classification, mode) of the picks on the n-th frame of a list: the classification alternates, the modes rotate"""
    return n % 2, DEPTH_MODES[n % 3]


_depth_draws = None


def depth_draws(oracle, vr):
    """Everything the depth tests draw, once, in a fixed order from DEPTH_STREAM: {"picks": {(list, n): [(x, y), ...]}, "partitions":
    [(n, mode, world, band_rows, x0, crop width)]}.  Picks: every pixel of a random frame of at most PICK_MAX pixels (nothing drawn), else
    the four corners and PICK_DRAWN drawn pixels.  Partitions: the first four random frames of a drawn permutation that are at least
    8 x 8 and have a surface in the frame's mode under both classifications; 2 or 3 ranks, bands of 1, 3 or 16 rows, a crop in x."""
    global _depth_draws
    if _depth_draws is None:
        rng = generator(DEPTH_STREAM)
        picks = {}
        for which in ("random", "holed"):
            for n, s, i, scene, f, opacity in depth_list(oracle, vr, which):
                w, h = f.p.view.width, f.p.view.height
                if which == "random" and w * h <= PICK_MAX:
                    picks[which, n] = [(x, y) for y in range(h) for x in range(w)]
                else:
                    picks[which, n] = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + \
                        [(int(x), int(y)) for x, y in zip(rng.integers(0, w, PICK_DRAWN), rng.integers(0, h, PICK_DRAWN))]
        frames = depth_list(oracle, vr, "random")
        partitions = []
        for n in (int(k) for k in rng.permutation(len(frames))):
            _, s, i, scene, f, opacity = frames[n]
            w, h = f.p.view.width, f.p.view.height
            mode = DEPTH_MODES[len(partitions) % 3]
            e = ExpectedDepth(scene, f, opacity)
            if w < 8 or h < 8 or not all(e.frame(cmode, mode).surface.any() for cmode in (0, 1)):
                continue
            x0 = int(rng.integers(0, w - 3))
            partitions.append((n, mode, int(rng.choice([2, 3])), int(rng.choice([1, 3, 16])), x0, int(rng.integers(1, w - x0 + 1))))
            if len(partitions) == 4:
                break
        _depth_draws = {"picks": picks, "partitions": partitions}
    return _depth_draws
