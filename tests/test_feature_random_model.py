"""CPU tier of the randomised and ragged-volume parity of the newer render features (tests/test_gpu_feature_random.py holds the GPU against
the restatements on the frames of tests/feature_random.py).  Here, on those same frames: the restatements agree with one another and with
the CPU oracle wherever two of them state the same thing — ties that the other *_model.py tests hold on the golden cases only — and the
frames are neither empty nor untouched by the feature they are meant to test, so the GPU tier cannot pass on frames that show nothing."""
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
    """every statement two restatements share, on one frame; returns the number of non-transparent pixels compared"""
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
