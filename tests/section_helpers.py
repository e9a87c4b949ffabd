"""Test-side helpers of the section tests: section_render and section_in_volume_render of tests/section_ref.c (the section frames of
include/vr_hip.h vr_hip_render_section / vr_hip_render_section_in_volume, restated with the CPU oracle's own statics on top of
tests/feature_ref.c), built through ref_library.compile_test_library, and the planes, slabs, windows and frame list both tiers use."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY
from light_helpers import LIT_VOLUMES, lit_views
from ref_library import Ref, SceneArgs, compile_test_library, frame_array, ptr
from slab_helpers import POINT as POINT_CLASSIFIED
from slab_helpers import slab_scene

SECTION_VOLUMES = LIT_VOLUMES                           # bucky, blob_40x24x56, random_u16, plateau
MODES = ("point", "max", "min", "mean")
MODE_NUMBER = {"point": 0, "max": 1, "min": 2, "mean": 3}
KX_LT_KC, MEAN_N_PLUS_1, MIN_FROM_0, THICK_DEPTH_KC = 1, 2, 3, 4      # the `perturb` of section_render: the sensitivity test's wrong readings
THICK_ON_KC = 5                                        # ... and the tie of the modes: a thick mode evaluated on POINT's segment [kc, kc]
# Half width of the thick frames, model units: 0.12, and at least 3.1 ray steps — a slab is at least 6 steps thick along its normal, so most
# of its rays hold several samples under the four-fold step too.  The plateau's block of 200 spans [-0.5, 0.5]^3 and is constant inside:
# its slabs are 0.62 either side, so that they straddle the block's faces and maximum, minimum and mean differ


def half_width_of(params, name):
    return PLATEAU_HALF_WIDTH if name == "plateau" else float(np.float32(max(0.12, 3.1 * params.ray_step)))


# The grey windows, raw voxel units: most of the range of each volume.  Bucky's starts at 0 and its MIN frames always take it: its transfer
# function is zero below a tenth of the range, so a slab minimum in the background is black whatever the minimum started from, while
# under a window from 0 every raw value of 1 or more shows
ALWAYS_WINDOWED = {("bucky", "min")}
WINDOWS = {"bucky": (0.0, 250.0), "blob_40x24x56": (10.0, 250.0), "random_u16": (2570.0, 64250.0), "plateau": (10.0, 250.0)}

PLATEAU_BOX = ((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6))
PLATEAU_TILT, TILT_AXIS = 0.8, (0.2672612, -0.5345225, 0.8017837)      # (1, -2, 3) / sqrt(14)
PLATEAU_HALF_WIDTH, PLATEAU_OFFSET = 0.36, 0.12

_library = None


def section_library():
    """tests/section_ref.c as a loaded library, built on first use"""
    global _library
    if _library is None:
        tmp = tempfile.mkdtemp(prefix="section_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _library = compile_test_library(tmp, "section_ref.c", "libsection_ref.so")
    return _library


def section_floats(plane, half_width, window):
    """plane[4], half_width, window lo, window hi: the seven floats of section_render"""
    lo, hi = (0.0, 0.0) if window is None else window
    return np.array(list(plane) + [half_width, lo, hi], np.float32)


class SectionRef(Ref):
    """section_render / section_in_volume_render of tests/section_ref.c on WHOLE frames; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.S = section_library()
        for f in (self.S.section_render, self.S.section_in_volume_render):
            f.restype = C.c_int

    def render(self, params, voxels, tf, plane, half_width=0.0, mode="point", window=None, clip=IDENTITY, perturb=0):
        """(RGBA frame, depth, samples per pixel — 0: a ray without a section, 0xffffffff: a ray that misses —, value per pixel)"""
        a = SceneArgs(params, voxels, tf, clip=clip)
        sec = section_floats(plane, half_width, window)

        def make():
            out, depth = frame_array(params, 4), frame_array(params, dtype=np.float32)
            count, value = frame_array(params, dtype=np.uint32), frame_array(params, dtype=np.float32)
            assert self.S.section_render(*a.base, a.clip, ptr(sec), C.c_uint32(MODE_NUMBER[mode]), C.c_uint32(perturb), ptr(out), ptr(depth), ptr(count), ptr(value)) == 0
            return out, depth, count, value
        return self.cached(("section",) + a.key + (sec.tobytes(), mode, int(perturb)), a.keep, make)

    def in_volume(self, params, voxels, tf, esl, plane, half_width=0.0, mode="point", window=None, cmode=POINT_CLASSIFIED, clip=IDENTITY, lighting=None,
                  q=None, strength=1.0):
        """(frame of the section inside the volume, the section's depth, the section frame)"""
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength, cmode)
        sec = section_floats(plane, half_width, window)

        def make():
            out, depth, section = frame_array(params, 4), frame_array(params, dtype=np.float32), frame_array(params, 4)
            assert self.S.section_in_volume_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, a.mode, ptr(sec), C.c_uint32(MODE_NUMBER[mode]), C.c_uint32(0),
                                                   ptr(out), ptr(depth), ptr(section)) == 0
            return out, depth, section
        return self.cached(("in_volume",) + a.key + (sec.tobytes(), mode), a.keep, make)


def unit(v):
    """v / |v| formed in double precision, as float32 values"""
    v = np.array(v, np.float64)
    v = v / np.sqrt((v ** 2).sum())
    return tuple(float(np.float32(c)) for c in v)


def planes_of(view, box=(None, None), tilt=0.0, offset=0.37):
    """The sections of one view, chosen by hand: (label, plane, clip).  The view's own direction through the centre (every ray that hits
    the cube carries a section), the diagonal (1,1,1) (or another of the four) through the centre and `offset` off it, the plane across z
    through the centre and `offset` off it, and `cut`: the first again with the context's clip plane ON the section — the volume cut open at
    the slice, where the clip has made kx == kc bit for bit.  A view that runs inside the plane across z (n . direction == 0: an all-miss
    frame by contract, tests/test_section_model.py has one) takes the plane across x or y instead.
    box, tilt, offset: for the plateau (PLATEAU_BOX, PLATEAU_TILT, PLATEAU_OFFSET: the sections off the centre still cross the block's middle).  Its block of 200 is constant and fills an eighth of the cube: the box is the
    crop box of the context's clip for all six, so that most section pixels lie on the block, and every normal is tilted by tilt * TILT_AXIS
    before it is normalised — a slab parallel to a face of the block, seen along an axis, holds the same voxels on every ray; a tilted one
    lies wholly inside the block on some rays (the minimum is 200) and straddles its faces on the others (maximum, minimum and mean differ)."""
    def tilted(n):
        return unit(tuple(c + tilt * t for c, t in zip(n, TILT_AXIS)))
    d = unit(tuple(view.direction))
    # (a view that looks almost along the (1,1,1) plane sees it as a thin stripe: it takes the first diagonal it looks at from 63 degrees or less)
    diagonal = next(n for n in (tilted(unit(c)) for c in ((1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, 1.0, -1.0))) if abs(np.dot(n, d)) >= 0.45)
    across = (0.0, 0.0, 1.0)
    if abs(d[2]) < 0.2:
        across = (1.0, 0.0, 0.0) if abs(d[0]) >= abs(d[1]) else (0.0, 1.0, 0.0)
    facing, across = tilted(d), tilted(across)
    open_clip = IDENTITY if box[0] is None else (box[0], box[1], None)
    return (
        ("facing", facing + (0.0,), open_clip),
        ("diagonal", diagonal + (0.0,), open_clip),
        ("diagonal_off", diagonal + (-offset,), open_clip),
        ("across", across + (0.0,), open_clip),
        ("across_off", across + (offset,), open_clip),
        ("cut", facing + (0.0,), (box[0], box[1], facing + (0.0,))),
    )


def tier_frames(vr, golden, oracle, volumes, name, sampling):
    """The frames of the GPU tier's main test for one (volume, sampling): nine views x the six sections of planes_of x the four modes; the
    colouring (transfer function / grey window) and the ray step (the volume's / four times it) alternate with view and section so that
    every mode meets all four combinations.  Yields (what, voxels, params, tf, plane, half_width, mode, window, clip); the CPU tier walks
    the same list."""
    for v, (label, view) in enumerate(lit_views(vr, golden, name)):
        for s, (section_label, plane, clip) in enumerate(planes_of(view, *((PLATEAU_BOX, PLATEAU_TILT, PLATEAU_OFFSET) if name == "plateau" else ()))):
            factor = 4 if (v + s) % 4 >= 2 else 1
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, True, factor)
            window = WINDOWS[name] if (v + s) % 2 == 0 else None
            for mode in MODES:
                shown = WINDOWS[name] if (name, mode) in ALWAYS_WINDOWED else window
                yield (name, sampling, label, section_label, mode, factor, shown is not None), vox, p, tf, plane, (0.0 if mode == "point" else half_width_of(p, name)), mode, shown, clip
