"""CPU tier of the depth frames and picks on the random, holed and edge-shape frames of tests/feature_random.py (tests/test_gpu_depth_random.py
holds the GPU against depth_render of tests/depth_ref.c on them).  Here, on those same frames and on the restatement alone: the depth
frame's alpha is tied to the composite restatements through the alpha byte, the three modes are held to the relations the contract implies
at the frames' own opacities and at the edges of (0, 1], and the frames are shown to carry surfaces, rays without one and whatever tells
the wrong readings of the contract apart — so the GPU tier cannot pass on frames that show nothing.  The caps are conditions on the
committed seed (VR_TEST_SEED), not measurements: a generator that misses one is tuned, the cap is not.  Every test prints what it counts."""
import hashlib

import numpy as np
import pytest

import feature_random as fr
from clip_helpers import ClipRef
from depth_helpers import ACC_BEFORE, MEAN_BY_ALPHA, MODES, PEAK_LAST, TERMINATOR_LOST, DepthRef, alpha_byte
from iso_helpers import depth_bits
from light_helpers import LightRef
from shadow_helpers import CUTOFF, ShadowRef
from slab_helpers import POINT, SLAB, SLAB_SKIPPED_IS_NONE, SlabRef

LISTS = ("random", "holed")
CMODES = ((POINT, "point"), (SLAB, "slab"))
WRONG = ((ACC_BEFORE, "ACC_BEFORE", "first"), (TERMINATOR_LOST, "TERMINATOR_LOST", "first"), (MEAN_BY_ALPHA, "MEAN_BY_ALPHA", "mean"), (PEAK_LAST, "PEAK_LAST", "peak"))


def same(a, b):
    return np.array_equal(depth_bits(a), depth_bits(b))


def edge_frames(oracle, vr):
    """(scene, frame, classification, {mode: opacity}, description) of the edge shapes as tests/test_gpu_depth.py test_edge_shapes renders them"""
    for dtype in fr.EDGE_DTYPES:
        for i, shape in enumerate(fr.EDGE_SHAPES):
            scene = fr.edge_scene(oracle, vr, shape, dtype)
            for j, f in enumerate(scene.frames):
                yield scene, f, (SLAB if (i + j) % 2 else POINT), {mode: (0.2, 0.6)[(i + m) % 2] for m, mode in enumerate(MODES)}, (shape, dtype, f.view, f.clip_name)


def check_alpha_tie(scene, f, opacity, what):
    """the alpha byte of the depth frame under the frame's clip, per classification, against the plain and the lit, shadowed composite
    restatements of that frame; returns the non-zero alpha bytes compared"""
    v, tf, esl = scene.vox, scene.tf, scene.esl
    clips, slab, light, shadow = ClipRef.instance(), SlabRef.instance(), LightRef.instance(), ShadowRef.instance()
    e = fr.ExpectedDepth(scene, f, opacity)
    q = shadow.build(f.light, f.S, f.shadow_step, v, tf, CUTOFF, f.shadow_sampling, clip=f.clip)
    composites = {POINT: (clips.composite(f.p, v, tf, esl, f.clip), light.render(f.p, v, tf, esl, f.lighting, q, f.strength, clip=f.clip)),     # (fr.Expected.lit)
                  SLAB: (slab.render(f.p, v, tf, esl, SLAB, f.clip), slab.render(f.p, v, tf, esl, SLAB, f.clip, f.lighting, q, f.strength))}    # (ExpectedLayers.slab_all)
    nonzero = 0
    for cmode, label in CMODES:
        d = e.frame(cmode, "first")
        assert all(same(e.frame(cmode, mode).alpha, d.alpha) for mode in MODES), (what, label, "the alpha depends on the mode")
        byte = alpha_byte(d.alpha)
        assert ((d.alpha >= 0.0) & (d.alpha <= 1.0)).all() and not byte[~d.segment].any(), (what, label)
        for k, frame in enumerate(composites[cmode]):
            assert np.array_equal(frame[..., 3], byte), (what, label, ("plain", "lit and shadowed")[k], int((frame[..., 3] != byte).sum()))
        nonzero += int((byte != 0).sum())
    return nonzero


def test_alpha_is_the_composites_alpha_byte(vr, oracle):
    """On every random, holed and edge-shape frame under its clip, for both classifications: map_float_int(alpha, 256) of the depth frame is
    the alpha byte of clip_render (point) or slab_render (slab), and of the same frame lit and shadowed as the frame's own lighting, light
    and strength have it (light_render: fr.Expected.lit; slab_render: ExpectedLayers.slab_all).  The alpha is the same bits in the three modes."""
    frames, nonzero = {}, {}
    for which in LISTS:
        for n, s, i, scene, f, opacity in fr.depth_list(oracle, vr, which):
            nonzero[which] = nonzero.get(which, 0) + check_alpha_tie(scene, f, opacity, (which, scene.describe(), i))
            frames[which] = frames.get(which, 0) + 1
    for scene, f, cmode, opacities, what in edge_frames(oracle, vr):
        nonzero["edge"] = nonzero.get("edge", 0) + check_alpha_tie(scene, f, 0.2, what)
        frames["edge"] = frames.get("edge", 0) + 1
    print(f"seed {fr.SEED}: alpha tie on {frames} frames, both classifications, plain and lit; non-zero alpha bytes compared: {nonzero}")
    assert frames == {"random": fr.SCENES * fr.FRAMES_PER_SCENE, "holed": fr.HOLED_SCENES * fr.HOLED_FRAMES, "edge": 6 * len(fr.EDGE_SHAPES) * len(fr.EDGE_DTYPES)}
    assert all(n > 1000 for n in nonzero.values()), nonzero


def test_the_frames_carry_surfaces_and_rays_without_one(vr, oracle):
    """Per list (random, holed), per classification and per mode: at least half of the frames carry a surface pixel at the frame's own
    opacity; at least half of the random frames, and every holed frame, hold a pixel that keeps a segment under the clip and has no surface
    in FIRST.  Printed beside them: the frames with a surface per mode and opacity, the surface pixels of PEAK, the segment pixels and the
    rays terminated above ray_threshold."""
    for which in LISTS:
        frames = fr.depth_list(oracle, vr, which)
        for cmode, label in CMODES:
            own = dict.fromkeys(MODES, 0)
            at = dict.fromkeys(fr.DEPTH_OPACITIES, 0)
            without = without_peak = pixels = segment = terminated = 0
            for n, s, i, scene, f, opacity in frames:
                e = fr.ExpectedDepth(scene, f, opacity)
                for mode in MODES:
                    own[mode] += int(e.frame(cmode, mode).surface.any())
                for o in fr.DEPTH_OPACITIES:
                    at[o] += int(e.frame(cmode, "first", o).surface.any())
                first, peak = e.frame(cmode, "first"), e.frame(cmode, "peak")
                without += int((first.segment & ~first.surface).any())
                without_peak += int((peak.segment & ~peak.surface).any())
                pixels, segment, terminated = pixels + int(peak.surface.sum()), segment + int(peak.segment.sum()), terminated + int(peak.terminated.sum())
            print(f"seed {fr.SEED}, {which}, {label}, of {len(frames)} frames — with a surface at the frame's opacity: {own}; FIRST at 0.1 / 0.5 / 0.9: {list(at.values())}; "
                  f"a segment pixel without a surface: FIRST {without}, PEAK {without_peak}; PEAK surface pixels {pixels}, segment pixels {segment}, terminated rays {terminated}")
            for mode in MODES:
                assert 2 * own[mode] >= len(frames), (which, label, mode, own[mode])
            assert without == len(frames) if which == "holed" else 2 * without >= len(frames), (which, label, without)


def test_mode_relations(vr, oracle):
    """On every random and holed frame, both classifications.  FIRST's surfaces shrink as the opacity grows over 0.1 / 0.5 / 0.9; PEAK and
    MEAN share one mask; at the smallest subnormal and the smallest normal opacity FIRST has a surface exactly where PEAK has one — where
    anything was composited; where ray_threshold < 1, FIRST at the next float32 above it has surfaces only on terminating samples
    (acc > threshold is the only way past the opacity) and exactly where FIRST at the threshold itself has them on this seed; opacity 1.0
    leaves surfaces in at least one random frame per classification."""
    for which in LISTS:
        for cmode, label in CMODES:
            at_one = at_one_px = at_threshold = at_threshold_px = terminated = 0
            for n, s, i, scene, f, opacity in fr.depth_list(oracle, vr, which):
                what = (which, label, scene.describe(), i)
                e = fr.ExpectedDepth(scene, f, opacity)
                ladder = [e.frame(cmode, "first", o).surface for o in fr.DEPTH_OPACITIES]
                for shallow, deep in zip(ladder, ladder[1:]):
                    assert not (deep & ~shallow).any(), what
                peak, mean = e.frame(cmode, "peak"), e.frame(cmode, "mean")
                assert np.array_equal(peak.surface, mean.surface), what
                edges = dict(fr.edge_opacities(f.p))
                for name in ("subnormal", "tiny"):
                    assert 0.0 < edges[name] and np.array_equal(e.frame(cmode, "first", edges[name]).surface, peak.surface), (what, name)
                one = e.frame(cmode, "first", edges["one"])
                at_one, at_one_px = at_one + int(one.surface.any()), at_one_px + int(one.surface.sum())
                if fr.THRESHOLD in edges:
                    assert f.p.ray_threshold < 1.0 and edges[fr.ABOVE_THRESHOLD] > edges[fr.THRESHOLD]
                    on, above = e.frame(cmode, "first", edges[fr.THRESHOLD]), e.frame(cmode, "first", edges[fr.ABOVE_THRESHOLD])
                    assert not (above.surface & ~above.terminated).any() and same(above.depth[above.surface], above.last[above.surface]), what
                    assert np.array_equal(above.surface, on.surface), what
                    at_threshold, at_threshold_px, terminated = at_threshold + int(on.surface.any()), at_threshold_px + int(on.surface.sum()), terminated + int(on.terminated.sum())
                else:
                    assert len(edges) == 3 and f.p.ray_threshold >= 1.0
            print(f"seed {fr.SEED}, {which}, {label}: FIRST at 1.0 has surfaces in {at_one} frames ({at_one_px} pixels); at ray_threshold in {at_threshold} "
                  f"frames ({at_threshold_px} pixels; {terminated} rays terminated there)")
            assert which != "random" or at_one >= 1, (label, at_one)


def changed_bits(e, mode, opacity, cmode=SLAB, perturb=0):
    """(depth, value, alpha) bits of the slab-classified frame change under this wrong reading"""
    a, b = e.frame(SLAB, mode, opacity), e.frame(cmode, mode, opacity, perturb)
    return not same(a.depth, b.depth), not same(a.value, b.value), not same(a.alpha, b.alpha)


def test_the_frames_tell_four_wrong_readings_apart(vr, oracle):
    """Sensitivity, under slab classification at opacity 0.5: FIRST testing acc before the update, the terminating sample not recorded
    (FIRST), MEAN divided by the final alpha, PEAK taking the last of equal peaks — each changes depth bits in at least a third of the
    random and of the holed frames"""
    for which in LISTS:
        frames = fr.depth_list(oracle, vr, which)
        changed = {}
        for n, s, i, scene, f, opacity in frames:
            e = fr.ExpectedDepth(scene, f, opacity)
            for perturb, name, mode in WRONG:
                changed[name] = changed.get(name, 0) + int(changed_bits(e, mode, 0.5, perturb=perturb)[0])
        print(f"seed {fr.SEED}: of {len(frames)} {which} frames, depth bits change under {changed}")
        for name, k in changed.items():
            assert 3 * k >= len(frames), (which, name, k)


def test_holed_scenes_reach_the_skipped_predecessor(vr, oracle):
    """The wrong reading SLAB_SKIPPED_IS_NONE of slab_colour — a sample the library may skip unresolved counts as no predecessor for the
    next one — at opacity 0.5: in every mode it changes depth, value or alpha bits in at least a third of the holed frames, as drawn and
    with esl = 0 / ray_threshold 1.0 (the march, not the leaping, meets the zero slab on every ray).  The random frames' count is printed
    for contrast: their volumes are smooth."""
    counts = {}
    for which in LISTS:
        frames = fr.depth_list(oracle, vr, which)
        for drawn in (True, False):
            for mode in MODES:
                any_bits, depth_only, alpha_only = 0, 0, 0
                for n, s, i, scene, f, opacity in frames:
                    e = fr.ExpectedDepth(scene, f, opacity, None if drawn else fr.full_march(f.p))
                    d, v, a = changed_bits(e, mode, 0.5, cmode=SLAB_SKIPPED_IS_NONE)
                    any_bits, depth_only, alpha_only = any_bits + int(d or v or a), depth_only + int(d or v), alpha_only + int(a)
                counts[which, drawn, mode] = any_bits
                print(f"seed {fr.SEED}: of {len(frames)} {which} frames {'as drawn' if drawn else 'with esl = 0 and threshold 1.0'}, {mode}: "
                      f"{depth_only} change depth or value bits, {alpha_only} alpha bits, {any_bits} any")
    holed = fr.HOLED_SCENES * fr.HOLED_FRAMES
    for (which, drawn, mode), k in counts.items():
        assert which != "holed" or 3 * k >= holed, (drawn, mode, k)


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_edge_shapes_have_surfaces(vr, oracle, dtype):
    """What test_edge_shapes of tests/test_gpu_depth.py rests on: every shape has, in every mode, a frame with a surface under the
    classification and at the opacity that test renders it with"""
    ref = DepthRef.instance()
    with_surface = {}
    for scene, f, cmode, opacities, what in edge_frames(oracle, vr):
        if what[1] != dtype:
            continue
        for mode in MODES:
            d = ref.render(f.p, scene.vox, scene.tf, scene.esl, opacities[mode], mode, cmode, f.clip)
            with_surface[what[0], mode] = with_surface.get((what[0], mode), 0) + int(d.surface.any())
    print(f"{dtype}: frames with a surface of 6 per (shape, mode):", {f"{'x'.join(map(str, k[0]))} {k[1]}": n for k, n in with_surface.items()})
    assert len(with_surface) == len(fr.EDGE_SHAPES) * 3 and all(n >= 1 for n in with_surface.values()), with_surface


def _fingerprint(oracle, vr):
    h = hashlib.sha256()
    for scenes in (fr.random_scenes(oracle, vr), fr.holed_scenes(oracle, vr)):
        for scene in scenes:
            h.update(scene.vox.tobytes() + np.asarray(scene.tf, np.float32).tobytes() + np.asarray(scene.esl, np.uint32).tobytes())
            for f in scene.frames:
                h.update(bytes(f.p) + bytes(f.mip) + bytes(f.iso) + repr((f.clip, f.S, f.light, f.shadow_step, f.shadow_sampling, f.strength, f.lighting, f.level,
                                                                            f.refine, f.clear_order)).encode())
    return h.hexdigest()


def test_the_new_stream_leaves_the_lists_alone(vr, oracle, monkeypatch):
    """The random and the holed lists drawn afresh — once with everything the depth tests draw (fr.depth_draws) drawn first, once without
    it — are, byte for byte (volumes, transfer functions, params and every per-frame setting), the lists of this session; DEPTH_STREAM is
    no other list's stream; at least six random frames have at most 256 pixels (one pick call covers them); and the picks' pixel lists
    hold hits, rays without a surface and rays that miss the cube."""
    session = _fingerprint(oracle, vr)
    draws = fr.depth_draws(oracle, vr)
    monkeypatch.setattr(fr, "_lists", {})
    monkeypatch.setattr(fr, "_depth_draws", None)
    again = fr.depth_draws(oracle, vr)
    with_draws = _fingerprint(oracle, vr)
    monkeypatch.setattr(fr, "_lists", {})
    without = _fingerprint(oracle, vr)
    monkeypatch.undo()
    assert session == with_draws == without and again == draws and fr.depth_draws(oracle, vr) is draws
    assert fr.DEPTH_STREAM not in (0, 1, 2, 3, 4, 5, 6, fr.HOLED_STREAM, 99, 411, 412, 611) and fr.DEPTH_STREAM % 1000 != 411
    small = [(f.p.view.width, f.p.view.height) for n, s, i, scene, f, opacity in fr.depth_list(oracle, vr, "random") if f.p.view.width * f.p.view.height <= fr.PICK_MAX]
    totals = {}
    for which in LISTS:
        hits = surface_misses = cube_misses = 0
        for n, s, i, scene, f, opacity in fr.depth_list(oracle, vr, which):
            pixels = draws["picks"][which, n]
            w, h = f.p.view.width, f.p.view.height
            assert len(pixels) == (w * h if which == "random" and w * h <= fr.PICK_MAX else 4 + fr.PICK_DRAWN) and len(pixels) <= fr.PICK_MAX
            assert all(0 <= x < w and 0 <= y < h for x, y in pixels)
            cmode, mode = fr.pick_state(n)
            d = fr.ExpectedDepth(scene, f, opacity).frame(cmode, mode)
            for x, y in pixels:
                hits, surface_misses, cube_misses = hits + int(d.surface[y, x]), surface_misses + int(d.rays[y, x] and not d.surface[y, x]), cube_misses + int(not d.rays[y, x])
        totals[which] = (hits, surface_misses, cube_misses)
    print(f"seed {fr.SEED}: {len(small)} random frames of at most {fr.PICK_MAX} pixels: {sorted(small)}; picks (hits, rays without a surface, rays that miss the cube): {totals}")
    print("partitions (frame, mode, ranks, band rows, x0, crop width):", draws["partitions"])
    assert len(small) >= 6, small
    assert all(min(t) > 0 for t in totals.values()), totals
    assert len(draws["partitions"]) == 4 and len({p[0] for p in draws["partitions"]}) == 4
