"""CPU tier of the randomised and ragged-volume parity of the newer render features (tests/test_gpu_feature_random.py holds the GPU against
the restatements on the frames of tests/feature_random.py).  Here, on those same frames: the restatements agree with one another and with
the CPU oracle wherever two of them state the same thing — ties that the other *_model.py tests hold on the golden cases only — and the
frames are neither empty nor untouched by the feature they are meant to test, so the GPU tier cannot pass on frames that show nothing.
Since tests/feature_ref.c states the feature ray, the MIP frame and the isosurface frame once, only the ties to clip_render and to the
oracle are between independent texts; the others compare two wrappers of one text, and tests/test_restatement_pins.py pins that text, on
these same frames, to the separate files it replaced."""
import numpy as np
import pytest

import feature_random as fr
from clip_helpers import IDENTITY, ClipRef
from iso_helpers import IsoRef, depth_bits
from light_helpers import IDENTITY_LIGHTING, LightRef, cue
from mip_helpers import MipRef
from shadow_helpers import ShadowRef


def edge_scenes(oracle, vr):
    return [(shape, dtype, fr.edge_scene(oracle, vr, shape, dtype)) for shape in fr.EDGE_SHAPES for dtype in fr.EDGE_DTYPES]


def check_ties(oracle, vr, scene, f, what):
    """every statement two restatements share, on one frame; returns the number of non-transparent pixels compared.  mip / clipped mip,
    iso / clipped iso and shadow / identity lighting are wrappers of one text each (tests/test_restatement_pins.py pins it); the composite
    against the oracle, and shadow and lighting against clip_render, are ties between independent texts"""
    clip_ref, mip_ref, iso_ref, shadow_ref, light_ref = ClipRef.instance(), MipRef.instance(), IsoRef.instance(), ShadowRef.instance(), LightRef.instance()
    v, tf, esl = scene.vox, scene.tf, scene.esl
    mip = mip_ref.render(f.mip, v, tf)[0]
    assert np.array_equal(clip_ref.mip(f.mip, v, tf, IDENTITY), mip), (what, "mip")
    iso, depth, _ = iso_ref.render(f.iso, v, tf, f.level, f.refine)
    clipped_iso = clip_ref.iso(f.iso, v, tf, f.level, f.refine, IDENTITY)
    assert np.array_equal(clipped_iso[0], iso) and np.array_equal(depth_bits(clipped_iso[1]), depth_bits(depth)), (what, "iso")
    skipped = iso_ref.render(f.iso, v, tf, f.level, f.refine, skipping=True)
    assert np.array_equal(skipped[0], iso) and np.array_equal(depth_bits(skipped[1]), depth_bits(depth)), (what, "iso skipping")
    plain = clip_ref.composite(f.p, v, tf, esl, IDENTITY)
    assert np.array_equal(plain, oracle.render(f.p, v, tf, esl, threads=4)), (what, "composite")
    for clip in (IDENTITY, f.clip):
        clipped = clip_ref.composite(f.p, v, tf, esl, clip)
        assert np.array_equal(shadow_ref.render(f.p, v, tf, esl, None, 1.0, clip), clipped), (what, "shadow without a grid", clip)
        assert np.array_equal(light_ref.render(f.p, v, tf, esl, IDENTITY_LIGHTING, clip=clip), clip_ref.composite(cue(f.p), v, tf, esl, clip)), (what, "identity lighting", clip)
    bound = f.mip if f.mip.sampling != vr.SAMPLE_NEAREST else fr.with_sampling(f.mip, vr.SAMPLE_TRILINEAR)
    assert mip_ref.bound_violations(bound, v)[0] == 0, (what, "mip bound")
    return int((plain[..., 3] != 0).sum()) + int((mip[..., 3] != 0).sum()) + int((depth >= 0).sum())


def test_the_generators_draw_what_they_promise(vr, oracle):
    """Independent of the seed's luck: 400 draws of each generator stay inside their domains and reach every special case"""
    rng = fr.generator(99)
    on_face = axis_normal = kinds = 0
    for _ in range(400):
        lo, hi, plane = fr.random_clip(rng)
        assert (lo is None) == (hi is None) and not (lo is None and plane is None)
        kinds |= (1 if lo is not None else 0) | (2 if plane is not None else 0) | (4 if lo is not None and plane is not None else 0)
        if lo is not None:
            assert all(-1.0 <= a < b <= 1.0 and b - a >= 0.49 for a, b in zip(lo, hi)), (lo, hi)
            on_face += int(any(a == -1.0 for a in lo) or any(b == 1.0 for b in hi))
        if plane is not None:
            assert abs(sum(c * c for c in plane[:3]) - 1.0) < 1e-5
            axis_normal += int(sorted(abs(c) for c in plane[:3]) == [0.0, 0.0, 1.0])
    assert kinds == 7 and on_face >= 40 and axis_normal >= 40, (kinds, on_face, axis_normal)
    nodes = faces = inside = 0
    for _ in range(400):
        S = int(rng.choice(fr.SHADOW_DIMS))
        light = fr.random_light(rng, S)
        grid = [-1.0 + 2.0 * i / (S - 1) for i in range(S)]
        nodes += int(all(c in grid for c in light))
        faces += int(any(abs(c) == 1.0 for c in light) and not all(c in grid for c in light))
        inside += int(all(abs(c) < 1.0 for c in light))
        ka, kd, ks, n = fr.random_lighting(rng)
        assert all(0.0 <= k <= 1.0 for k in (ka, kd, ks)) and 0 <= n <= 10
    assert nodes >= 40 and faces >= 40 and inside >= 100, (nodes, faces, inside)
    assert fr.clamp_step(0.0) == fr.MIN_STEP and fr.clamp_step(0.3) == float(np.float32(0.3))
    for scene in fr.random_scenes(oracle, vr):
        for f in scene.frames:
            assert f.p.ray_step >= fr.MIN_STEP and f.shadow_step >= fr.MIN_STEP and f.p.sampling in (1, 2) and f.iso.sampling in (1, 2)
            nz = scene.vox[scene.vox > 0]
            assert nz.min() <= f.level <= nz.max() + 0.5
    assert (1, 1, 1) not in fr.EDGE_SHAPES
    for shape, dtype, scene in edge_scenes(oracle, vr):
        assert scene.vox.shape == shape[::-1] and all(f.p.ray_step >= fr.MIN_STEP for f in scene.frames)
        assert scene.vox.min() < 128 * (257 if dtype == "uint16" else 1) < scene.vox.max() and len(scene.frames) == 6


def test_restatements_agree_on_the_random_frames(vr, oracle):
    """MIP, isosurface (RGBA and depth bits, with and without the skipping emulation), composite, shadow without a grid, identity lighting
    and the MIP's skip bound on every random frame the GPU tier renders"""
    compared = frames = inside = axis = 0
    for scene in fr.random_scenes(oracle, vr):
        for i, f in enumerate(scene.frames):
            compared += check_ties(oracle, vr, scene, f, (scene.describe(), i))
            frames += 1
            inside += int(f.camera_inside())
            axis += int(f.axis_aligned())
    print(f"{frames} random frames, {inside} with the camera inside the cube, {axis} along an axis; {compared} covered pixels compared")
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE and compared > 1000
    assert inside >= 4 and axis >= 4, (inside, axis)           # what the GPU tier asserts of its frames too


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_restatements_agree_on_the_edge_shapes(vr, oracle, dtype):
    compared = 0
    for shape in fr.EDGE_SHAPES:
        scene = fr.edge_scene(oracle, vr, shape, dtype)
        for f in scene.frames:
            compared += check_ties(oracle, vr, scene, f, (shape, dtype, f.view, f.clip_name))
    print(f"{dtype}: {compared} covered pixels compared on {len(fr.EDGE_SHAPES)} shapes")
    assert compared > 1000


def _shares(scene, f):
    """(non-empty per family, feature shown per family) of one frame, from the restatements alone"""
    e = fr.Expected(scene, f)
    clip_ref, shadow_ref = ClipRef.instance(), ShadowRef.instance()
    v, tf, esl = scene.vox, scene.tf, scene.esl
    nonempty = {"composite": e.composite.any(), "mip": e.mip.any(), "iso": e.iso.any(), "shadowed": e.shadowed.any(), "lit": e.lit.any()}
    shown = {"clip changes the composite": not np.array_equal(e.composite, clip_ref.composite(f.p, v, tf, esl, IDENTITY)),
             "isosurface with 20 hits": int((e.depth >= 0).sum()) >= 20,
             "grid byte between 0 and 255": bool(((e.q > 0) & (e.q < 255)).any()),
             "shadow changes the frame": not np.array_equal(e.shadowed, e.composite),
             "lighting changes the frame": not np.array_equal(e.lit, e.shadowed)}
    return {k: bool(x) for k, x in nonempty.items()}, shown, e


def test_random_frames_hold_the_caps(vr, oracle):
    """Conditions, not measurements, on the committed seed's frames: per family at least half of the frames have a non-zero pixel, and at
    least one third show the feature — the clipped composite differs from the unclipped one, the isosurface has 20 hit pixels or more, the
    light grid holds a byte strictly between 0 and 255, the shadowed frame differs from the unshadowed one, the lit frame from the cue-lit
    one (both under the same shadow).  A generator that misses a cap is tuned; the cap is not."""
    nonempty, shown, frames = {}, {}, 0
    for scene in fr.random_scenes(oracle, vr):
        for f in scene.frames:
            a, b, _ = _shares(scene, f)
            for k, x in a.items():
                nonempty[k] = nonempty.get(k, 0) + int(x)
            for k, x in b.items():
                shown[k] = shown.get(k, 0) + int(x)
            frames += 1
    print(f"seed {fr.SEED}, of {frames} frames — non-empty:", ", ".join(f"{k} {n}" for k, n in nonempty.items()))
    print("feature shown:", ", ".join(f"{k} {n}" for k, n in shown.items()))
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE
    for k, n in nonempty.items():
        assert 2 * n >= frames, (k, n, frames)
    for k, n in shown.items():
        assert 3 * n >= frames, (k, n, frames)


def test_edge_shapes_hold_the_caps(vr, oracle):
    """Every shape, u8 and u16: in every family at least one of the shape's six frames is not empty, and some dense sample of the lit frames
    has a non-zero gradient (LightRef's counters: dense > flat)"""
    for shape, dtype, scene in edge_scenes(oracle, vr):
        nonempty, dense, flat, hits = {}, 0, 0, 0
        for f in scene.frames:
            a, _, e = _shares(scene, f)
            for k, x in a.items():
                nonempty[k] = nonempty.get(k, 0) + int(x)
            dense += e.dense
            flat += e.flat
            hits += int((e.depth >= 0).sum())
        print(f"{shape} {dtype}: non-empty of {len(scene.frames)} frames", nonempty, f"; {hits} isosurface hits, {dense} dense samples, {flat} with a zero gradient")
        assert all(n >= 1 for n in nonempty.values()), (shape, dtype, nonempty)
        assert dense > flat, (shape, dtype, dense, flat)


# ---- slab, backdrop and hybrid frames on the same random frames and edge shapes (fr.ExpectedLayers) ----

def random_layer_frames(oracle, vr):
    """(scene, frame, salt of its synthetic layer, description) of the 56 random frames"""
    for s, scene in enumerate(fr.random_scenes(oracle, vr)):
        for i, f in enumerate(scene.frames):
            yield scene, f, fr.layer_salt(s, i), (scene.describe(), i)


def edge_layer_frames(oracle, vr):
    for n, (shape, dtype, scene) in enumerate(edge_scenes(oracle, vr)):
        for i, f in enumerate(scene.frames):
            yield scene, f, fr.EDGE_SALT + 8 * n + i, (shape, dtype, f.view, f.clip_name)


def check_layer_ties(scene, f, salt, what):
    """every statement slab_render, backdrop_render and hybrid_render share with the older restatements, on one frame under its clip;
    returns the number of non-transparent pixels compared.  Only the tie to clip_render is between two texts; the rest compares wrappers
    of one ray and one isosurface frame (tests/test_restatement_pins.py pins them)"""
    from backdrop_helpers import BackdropRef
    from slab_helpers import POINT, SLAB, SlabRef
    clip_ref, slab_ref, ref = ClipRef.instance(), SlabRef.instance(), BackdropRef.instance()
    v, tf, esl = scene.vox, scene.tf, scene.esl
    e = fr.ExpectedLayers(scene, f, salt)
    point = slab_ref.render(f.p, v, tf, esl, POINT, f.clip)
    assert np.array_equal(point, clip_ref.composite(f.p, v, tf, esl, f.clip)), (what, "slab restatement, point classified")
    shape = e.depth.shape
    for mode, want, none in ((POINT, point, np.full(shape, -1.0, np.float32)), (SLAB, e.slab, np.full(shape, np.nan, np.float32))):
        assert np.array_equal(ref.render(f.p, v, tf, esl, None, None, mode, f.clip), want), (what, "backdrop without a layer", mode)
        assert np.array_equal(ref.render(f.p, v, tf, esl, e.rgba, none, mode, f.clip), want), (what, "backdrop without a surface", mode)
    iso, depth, _ = clip_ref.iso(f.p, v, tf, f.level, f.refine, f.clip)
    assert np.array_equal(e.hybrid_iso, iso) and np.array_equal(depth_bits(e.hybrid_depth), depth_bits(depth)), (what, "the hybrid's isosurface")
    assert np.array_equal(e.hybrid, ref.render(f.p, v, tf, esl, iso, depth, POINT, f.clip)), (what, "hybrid = backdrop over the isosurface")
    return int((point[..., 3] != 0).sum()) + int((e.slab[..., 3] != 0).sum()) + int((depth >= 0).sum())


def test_slab_and_backdrop_restatements_agree_on_the_random_frames(vr, oracle):
    """On all 56 random frames, byte for byte: the point-classified slab restatement is the clipped composite; a backdrop frame without a
    layer, or with the synthetic layer's colours under a depth layer of all -1 (point) or all NaN (slab), is the frame without one; the
    hybrid's isosurface frame and depth bits are clip_iso_render's and the hybrid is the backdrop frame over them"""
    compared = frames = 0
    for scene, f, salt, what in random_layer_frames(oracle, vr):
        compared += check_layer_ties(scene, f, salt, what)
        frames += 1
    print(f"{frames} random frames; {compared} covered pixels compared")
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE and compared > 1000


def test_slab_and_backdrop_restatements_agree_on_the_edge_shapes(vr, oracle):
    compared = frames = 0
    for scene, f, salt, what in edge_layer_frames(oracle, vr):
        compared += check_layer_ties(scene, f, salt, what)
        frames += 1
    print(f"{frames} edge frames; {compared} covered pixels compared")
    assert frames == 6 * len(fr.EDGE_SHAPES) * len(fr.EDGE_DTYPES) and compared > 1000


def test_random_wide_slabs_lose_nothing_to_cancellation(vr, oracle):
    """The bound of tests/test_slab_model.py test_wide_slabs_lose_nothing_to_cancellation, on the sum over the 56 random frames under their
    clips: the fp32 wide-slab branch against the same branch in double precision — no byte differs by more than 1 and at most 0.1 % of the
    non-empty pixels differ.  And the integral table of each of the 14 random transfer functions: within 128 roundings of values below
    128 (2^-17 each) of the float64 cumulative trapezoid sum, and exactly 0 through the leading zeros."""
    from slab_helpers import SLAB, SLAB_DOUBLE, SlabRef
    ref = SlabRef.instance()
    nonempty = differ = worst = 0
    for scene, f, _, what in random_layer_frames(oracle, vr):
        single = ref.render(f.p, scene.vox, scene.tf, scene.esl, SLAB, f.clip)
        double = ref.render(f.p, scene.vox, scene.tf, scene.esl, SLAB_DOUBLE, f.clip)
        nonempty += int(double.any(axis=-1).sum())
        differ += int((single != double).any(axis=-1).sum())
        worst = max(worst, int(np.abs(single.astype(int) - double.astype(int)).max(initial=0)))
    print(f"seed {fr.SEED}: {differ} of {nonempty} non-empty pixels differ from the double-precision frame, worst byte {worst}")
    assert nonempty > 1000 and worst <= 1 and differ <= 0.001 * nonempty, (worst, differ, nonempty)
    off = 0.0
    for scene in fr.random_scenes(oracle, vr):
        tf = np.asarray(scene.tf, np.float32).reshape(128, 4)
        K = ref.integral(tf)
        exact = np.concatenate([np.zeros((1, 4)), np.cumsum(0.5 * (tf[:-1].astype(np.float64) + tf[1:].astype(np.float64)), axis=0)])
        off = max(off, float(np.abs(K - exact).max()))
        zeros = 0
        while zeros < 128 and not tf[zeros].any():
            zeros += 1
        assert K.shape == (128, 4) and not K[:max(zeros, 1)].any(), (scene.describe(), zeros)
    print(f"integral tables of the {fr.SCENES} random transfer functions: at most {off:.2e} from the float64 sums")
    assert off <= 128 * 2.0 ** -17, off


def test_random_layer_frames_hold_the_caps(vr, oracle):
    """Conditions, not measurements, on the committed seed's frames.  At least half of the slab and of the backdrop frames have a non-zero
    pixel.  At least a third of the frames: differ from the point-classified frame; take the wide-slab branch on a fifth or more of their
    accumulating samples; change under lighting, light grid and strength; have a surface pixel that differs from the layer's colour word;
    have 20 or more surface pixels that differ from both the layer and the plain composite; have 20 or more surface pixels in the hybrid.
    At least a fifth have 20 or more surface pixels of the hybrid that differ from both the isosurface frame and the plain composite: random
    holed transfer functions leave the matter in front of many surfaces transparent, whatever the level.  A salt or a generator that
    misses a cap is tuned; the cap is not."""
    from slab_helpers import POINT, SlabRef
    slab_ref = SlabRef.instance()
    nonempty = {"slab": 0, "backdrop": 0}
    third = {"slab differs from point": 0, "a fifth of the samples are wide slabs": 0, "the states change the slab frame": 0,
             "a surface pixel differs from the layer": 0, "20 surface pixels differ from layer and composite": 0, "hybrid with 20 surface pixels": 0}
    fifth = {"20 hybrid surface pixels differ from isosurface and composite": 0}
    frames = 0

    def differs(a, b):
        return (a != b).any(axis=-1)
    for scene, f, salt, what in random_layer_frames(oracle, vr):
        e = fr.ExpectedLayers(scene, f, salt)
        point = slab_ref.render(f.p, scene.vox, scene.tf, scene.esl, POINT, f.clip)
        surface, hit = e.depth >= 0, e.hybrid_depth >= 0
        assert e.samples == e.wide + e.narrow
        nonempty["slab"] += int(e.slab.any())
        nonempty["backdrop"] += int(e.backdrop.any())
        for k, x in zip(third, (not np.array_equal(e.slab, point), e.samples > 0 and 5 * e.wide >= e.samples, not np.array_equal(e.slab_all, e.slab),
                                (differs(e.backdrop, e.rgba) & surface).any(),
                                int((differs(e.backdrop, e.rgba) & differs(e.backdrop, point) & surface).sum()) >= 20, int(hit.sum()) >= 20)):
            third[k] += int(bool(x))
        for k in fifth:
            fifth[k] += int(int((differs(e.hybrid, e.hybrid_iso) & differs(e.hybrid, point) & hit).sum()) >= 20)
        frames += 1
    print(f"seed {fr.SEED}, of {frames} frames — non-empty:", ", ".join(f"{k} {n}" for k, n in nonempty.items()))
    print("shown:", ", ".join(f"{k} {n}" for k, n in {**third, **fifth}.items()))
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE
    for k, n in nonempty.items():
        assert 2 * n >= frames, (k, n, frames)
    for k, n in third.items():
        assert 3 * n >= frames, (k, n, frames)
    for k, n in fifth.items():
        assert 5 * n >= frames, (k, n, frames)


def test_edge_shape_hybrids_hold_the_cap(vr, oracle):
    """Every shape, u8 and u16: the six hybrid frames under all four states together have 100 or more surface pixels that differ from the
    isosurface frame — the matter in front of the surface contributes"""
    least = None
    for shape, dtype, scene in edge_scenes(oracle, vr):
        shown = 0
        for f in scene.frames:
            e = fr.ExpectedLayers(scene, f)
            shown += int(((e.hybrid_all != e.hybrid_iso).any(axis=-1) & (e.hybrid_depth >= 0)).sum())
        print(f"{shape} {dtype}: {shown} surface pixels of the six all-states hybrids differ from the isosurface frame")
        assert shown >= 100, (shape, dtype, shown)
        least = shown if least is None else min(least, shown)
    print("least:", least)


def test_random_backdrop_frames_tell_three_wrong_readings_apart(vr, oracle):
    """Sensitivity, as tests/test_backdrop_model.py has it on the golden frames: the restatement perturbed three ways — a sample at k == d
    not composited, the layer not blended in once early termination has struck, bf = byte / 255 — changes at least one of the 56 random
    backdrop frames each"""
    from backdrop_helpers import BYTE_OVER_255, K_LT_D, NO_BLEND_AFTER_ERT, BackdropRef
    from slab_helpers import POINT
    ref = BackdropRef.instance()
    changed = {K_LT_D: 0, NO_BLEND_AFTER_ERT: 0, BYTE_OVER_255: 0}
    frames = 0
    for scene, f, salt, what in random_layer_frames(oracle, vr):
        e = fr.ExpectedLayers(scene, f, salt)
        for perturb in changed:
            changed[perturb] += int(not np.array_equal(e.backdrop, ref.render(f.p, scene.vox, scene.tf, scene.esl, e.rgba, e.depth, POINT, f.clip, perturb=perturb)))
        frames += 1
    print(f"of {frames} backdrop frames: {changed[K_LT_D]} change under k < d, {changed[NO_BLEND_AFTER_ERT]} without the blend after early termination, "
          f"{changed[BYTE_OVER_255]} under byte / 255")
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE
    for perturb, n in changed.items():
        assert n >= 1, (perturb, n)


def holed_layer_frames(oracle, vr):
    for s, scene in enumerate(fr.holed_scenes(oracle, vr)):
        for i, f in enumerate(scene.frames):
            yield scene, f, fr.layer_salt(200 + s, i), (scene.describe(), i)


def test_holed_scenes_reach_the_skipped_predecessor(vr, oracle):
    """The holed scenes (fr.holed_scenes: a slab of exact zeros through a random volume) hold the ties of the random frames, and at least a
    third of their slab frames change under the wrong reading SLAB_SKIPPED_IS_NONE of slab_render — a sample the library may skip
    unresolved counts as no predecessor for the next one.  On the 56 random frames that reading changes 5: their volumes are smooth, and
    a value seldom jumps from what may be skipped to what shows within one step.  The reading is per ray; the library skips per wave."""
    from slab_helpers import SLAB, SLAB_SKIPPED_IS_NONE, SlabRef
    ref = SlabRef.instance()
    frames = changed = compared = 0
    for scene, f, salt, what in holed_layer_frames(oracle, vr):
        compared += check_layer_ties(scene, f, salt, what)
        e = fr.ExpectedLayers(scene, f, salt)
        changed += int(not np.array_equal(e.slab, ref.render(f.p, scene.vox, scene.tf, scene.esl, SLAB_SKIPPED_IS_NONE, f.clip)))
        frames += 1
        assert min(f.p.view.width, f.p.view.height) >= 16 and not scene.vox.all()
    smooth = sum(int(not np.array_equal(ref.render(f.p, s.vox, s.tf, s.esl, SLAB, f.clip), ref.render(f.p, s.vox, s.tf, s.esl, SLAB_SKIPPED_IS_NONE, f.clip)))
                 for s, f, _, _ in random_layer_frames(oracle, vr))
    print(f"{changed} of {frames} holed slab frames change when a skipped predecessor counts as none ({smooth} of the 56 random frames); "
          f"{compared} covered pixels compared")
    assert frames == fr.HOLED_SCENES * fr.HOLED_FRAMES and compared > 1000
    assert 3 * changed >= frames, (changed, frames)
