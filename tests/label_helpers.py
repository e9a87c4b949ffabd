"""Test-side helpers of the label tests: label_render of tests/label_ref.c (the labelled composite frame of include/vr_hip.h
vr_hip_render_labelled, restated with the CPU oracle's own statics on top of tests/feature_ref.c), built through
ref_library.compile_test_library; the label volumes and the table both tiers use; the frame list both tiers walk; and what the GPU tiers do
with one frame (set_state, check)."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import CLIPS, IDENTITY, set_clip
from light_helpers import LIT_VOLUMES, PHONG, lit_views
from ref_library import Ref, SceneArgs, compile_test_library, contiguous, frame_array, ptr
from shadow_helpers import CUTOFF, LIGHTS, ShadowRef
from slab_helpers import slab_scene

LABEL_VOLUMES = LIT_VOLUMES                             # bucky, blob_40x24x56, random_u16, plateau
FLOOR, AFTER_SHADING, ALPHA_ONLY, MIX_SCALED = 1, 2, 3, 4       # the `perturb` of label_render: the sensitivity test's wrong readings
PERTURBATIONS = (FLOOR, AFTER_SHADING, ALPHA_ONLY, MIX_SCALED)
# the five kinds of entry every table of the tests holds, entry i being of kind i % 5
IDENTITY_KIND, HIDDEN, REPLACED, TINTED, FADED = range(5)
KINDS = ("identity", "hidden", "mix 1", "fractional mix", "fractional opacity")
SHADINGS = ("cue", "lit", "shadowed", "lit + shadowed")
SHADOW = ("top", 17, 0.6)                               # the light, the grid's nodes per edge and the strength of the shadowed frames
_CLIP_CYCLE = (IDENTITY, CLIPS["box"], CLIPS["plane"], CLIPS["both"])
_CLIP_NAMES = ("identity", "box", "plane", "both")


def table(entries=256):
    """(entries, 5) float32 of { colour[3], mix, opacity }: entry i is of kind i % 5 — identity, hidden (opacity 0), mix 1, a fractional mix,
    a fractional opacity (with and without a mix) —, its colour and its fractions drawn from i alone (binary fractions of 64: every member is an exact float)"""
    t = np.zeros((entries, 5), np.float32)
    for i in range(entries):
        kind = i % 5
        colour = [((17 * i + 5) % 64) / 64.0, ((29 * i + 11) % 64) / 64.0, ((43 * i + 23) % 64) / 64.0]
        mix, opacity = 0.0, 1.0
        if kind == HIDDEN:
            mix, opacity = ((7 * i) % 64) / 64.0, 0.0
        elif kind == REPLACED:
            mix = 1.0
        elif kind == TINTED:
            mix = (8 + (11 * i) % 48) / 64.0
        elif kind == FADED:                             # every second one tinted too: colour times the scaled or the unscaled alpha differ there
            mix, opacity = ((i // 5 + 1) % 2) * (8 + (19 * i) % 48) / 64.0, (8 + (13 * i) % 48) / 64.0
        t[i] = colour + [mix, opacity]
    return t


def identity_table(entries=256):
    t = np.zeros((entries, 5), np.float32)
    t[:, 4] = 1.0
    return t


def constant_table(mix, opacity, colour=(0.0, 0.0, 0.0), entries=256):
    t = np.zeros((entries, 5), np.float32)
    t[:] = list(colour) + [mix, opacity]
    return t


_labels = {}


def structured_labels(vox):
    """Five labels made from the volume's shape alone: slanted stripes five voxels thick along (3, 2, 1) — they cross every cell off-axis —
    carrying labels 0..3, and a ball around the centre, a third of the smallest extent in radius, carrying 4"""
    key = ("structured", vox.shape)
    if key not in _labels:
        z, y, x = vox.shape
        zz, yy, xx = np.mgrid[0:z, 0:y, 0:x]
        lab = (((3 * xx + 2 * yy + zz) // 5) % 4).astype(np.uint8)
        r = max(min(x, y, z) / 3.0, 1.0)
        ball = (xx - (x - 1) / 2.0) ** 2 + (yy - (y - 1) / 2.0) ** 2 + (zz - (z - 1) / 2.0) ** 2 <= r * r
        lab[ball] = 4
        lab = np.ascontiguousarray(lab)
        lab.setflags(write=False)
        _labels[key] = lab
    return _labels[key]


def random_labels(vox, salt=0):
    """One uniform label of 0..255 per voxel, from the shape and the salt alone: an off-by-one in an index or a brick address changes bytes"""
    key = ("random", vox.shape, salt)
    if key not in _labels:
        z, y, x = vox.shape
        rng = np.random.default_rng([20261020, x, y, z, salt])
        lab = rng.integers(0, 256, size=vox.shape, dtype=np.uint8)
        lab.setflags(write=False)
        _labels[key] = lab
    return _labels[key]


def labels_for(name, vox):
    """the label volume of a test volume: random on the random volume, structured elsewhere"""
    return random_labels(vox) if name.startswith("random") else structured_labels(vox)


_library = None


def label_library():
    """tests/label_ref.c as a loaded library, built on first use"""
    global _library
    if _library is None:
        tmp = tempfile.mkdtemp(prefix="label_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _library = compile_test_library(tmp, "label_ref.c", "liblabel_ref.so")
    return _library


class LabelFrame:
    """label_render's answers for one frame: the frame, the samples of every pixel's accumulation loop, and per label the samples of the
    loops whose looked-up alpha is above 0"""

    def __init__(self, frame, count, by_label):
        self.frame, self.count, self.by_label = frame, count, by_label

    def by_kind(self):
        return np.array([int(self.by_label[k::5].sum()) for k in range(5)], np.int64)


class LabelRef(Ref):
    """label_render of tests/label_ref.c on WHOLE frames; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.D = label_library()
        self.D.label_render.restype = C.c_int

    def render(self, params, voxels, tf, esl, labels, entries, lighting=None, q=None, strength=1.0, clip=IDENTITY, perturb=0):
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength)
        lab = contiguous(labels, np.uint8)
        assert lab.shape == np.asarray(voxels).shape
        full = identity_table()
        ent = np.asarray(entries, np.float32).reshape(-1, 5)
        full[: ent.shape[0]] = ent

        def make():
            out, count, by_label = frame_array(params, 4), frame_array(params, dtype=np.uint32), np.zeros(256, np.uint64)
            assert self.D.label_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, ptr(lab), ptr(full), C.c_uint32(perturb), ptr(out), ptr(count), ptr(by_label)) == 0
            return (LabelFrame(out, count, by_label),)
        return self.cached(("label",) + a.key + (lab.ctypes.data, full.tobytes(), int(perturb)), a.keep + (lab,), make)[0]


def shadow_grid(vox, tf, p, clip):
    """the light grid of the shadowed frames: SHADOW's light and size, the frame's ray step and sampling, under the frame's clip (None: none set)"""
    return ShadowRef.instance().build(LIGHTS[SHADOW[0]], SHADOW[1], float(p.ray_step), vox, tf, CUTOFF, 1, clip=clip)


class Case:
    """One frame of the lists: what is rendered (vox, p, tf, esl), under which clip (`clip` what the restatement takes, `set_clip` what the
    context is given: None = none set), lighting (None: the cue) and shadow (q None: none; `shadow` = the light, the grid's nodes per edge, the
    builder's step and sampling the context is given, `strength` its strength)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def tier_frames(vr, golden, oracle, volumes, name, sampling):
    """The scenes of both tiers' main tests for one (volume, sampling): the nine views of lit_views, two frames each — 18 frames whose
    shading (cue, lit, shadowed, lit + shadowed), clip (identity, box, plane, both), mode (default / full march) and ray step (x1 / x4) are
    arranged so that every pair of settings meets (tests/test_label_model.py asserts it)."""
    for i in range(18):
        label, view = lit_views(vr, golden, name)[i // 2]
        shading, k, full, fourfold = i % 4, (i // 4 + i % 4) % 4, (i // 4) % 2, (i // 8) % 2
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, bool(full), 4 if fourfold else 1)
        if not full and p.ray_threshold >= 1.0:         # (the blob's golden state never terminates a ray: its default-mode frames take 0.95 here)
            p = p.copy()
            p.ray_threshold = 0.95
        set_to = None if k == 0 else _CLIP_CYCLE[k]
        yield Case(what=(name, sampling, label, SHADINGS[shading], _CLIP_NAMES[k], "full" if full else "default", 4 if fourfold else 1),
                   settings=(shading, k, full, fourfold), vox=vox, p=p, tf=tf, esl=esl, clip=_CLIP_CYCLE[k], set_clip=set_to,
                   lighting=PHONG if shading in (1, 3) else None, q=shadow_grid(vox, tf, p, set_to) if shading >= 2 else None,
                   shadow=(LIGHTS[SHADOW[0]], SHADOW[1], float(p.ray_step), 1), strength=SHADOW[2])


# ---- what the GPU tiers (tests/test_gpu_label.py, tests/test_gpu_label_random.py) do with one frame ----

def label_launch(info):
    """what every labelled frame's launch looks like: what a depth frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


def set_state(gpu, case):
    """the context's clip, lighting and shadow as the case has them"""
    if case.set_clip is None:
        gpu.clear_clip()
    else:
        set_clip(gpu, case.set_clip)
    if case.lighting is None:
        gpu.clear_lighting()
    else:
        gpu.set_lighting(*case.lighting)
    if case.q is None:
        gpu.clear_shadow()
    else:
        light, dims, step, sampling = case.shadow
        gpu.set_shadow(light, dims, float(step), float(case.strength), CUTOFF, sampling)


def check(gpu, ref, case, labels, entries):
    """the host entry point against label_render: bytes; returns the restatement's frame.  Labels and table are the caller's business."""
    want = ref.render(case.p, case.vox, case.tf, case.esl, labels, entries, case.lighting, case.q, case.strength, case.clip)
    got = gpu.render_labelled(case.p)
    info = gpu.last_launch()
    wrong = int((got != want.frame).any(axis=-1).sum())
    assert wrong == 0, (case.what, wrong, info)
    assert label_launch(info), (case.what, info)
    return want


def random_case(scene, i, f, shading):
    """the Case of frame i of a scene of tests/feature_random.py under its own clip, with its own lighting and shadow where `shading` asks"""
    lit, shadowed = shading in (1, 3), shading >= 2
    q = ShadowRef.instance().build(f.light, f.S, f.shadow_step, scene.vox, scene.tf, CUTOFF, f.shadow_sampling, clip=f.clip) if shadowed else None
    return Case(what=(scene.describe(), "frame", i, SHADINGS[shading], "persp", f.p.view.perspective, (f.p.view.width, f.p.view.height)),
                vox=scene.vox, p=f.p, tf=scene.tf, esl=scene.esl, clip=f.clip, set_clip=f.clip, lighting=tuple(f.lighting) if lit else None, q=q,
                shadow=(f.light, f.S, f.shadow_step, f.shadow_sampling), strength=float(f.strength))
