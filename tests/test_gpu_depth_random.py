"""Random, holed and ragged parity of the depth frames and of picking (vr_hip_render_depth*, vr_hip_pick): the 14 x 4 random frames and the
holed scenes of tests/feature_random.py — frames of 1 x 8 to 69 x 49 pixels, cameras inside the cube, exact zeros in the direction, the
four-fold ray step, random transfer functions with holes and leading zeros, a slab of exact zeros through the volume, a random clip, block
grid and threshold, layout and wide addressing alternating per scene — held bit for bit, no tolerance anywhere, against depth_render of
tests/depth_ref.c: depth, value and alpha, at the frames' own opacities and at the edges of (0, 1], the picks of every pixel of the small
frames, the FIRST depth as a backdrop layer, band partitions and crops.  tests/test_depth_random_model.py ties the restatement to the
composite restatements on these frames and shows that they carry surfaces, rays without one and what tells the wrong readings apart.
Other seeds: VR_TEST_SEED=... pytest -m gpu tests/test_gpu_depth_random.py"""
import numpy as np
import pytest

import feature_random as fr
from backdrop_helpers import BackdropRef
from clip_helpers import set_clip
from depth_helpers import MODES, DepthRef, alpha_byte, check, classify, depth_launch
from gpu_feature import depth_diff, diff, expected_bands, load, needs_bounds_lib, reset_context, run_under_bounds_build
from shadow_helpers import CUTOFF
from slab_helpers import POINT, SLAB

pytestmark = pytest.mark.gpu

LISTS = ("random", "holed")
WINDOW = (70, 50)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout or a forced path behind"""
    yield
    reset_context(vr, gpu)


def scenes_of(oracle, vr, which):
    """[(scene index, scene, [(n, frame index, frame, opacity)])] of a list"""
    out = {}
    for n, s, i, scene, f, opacity in fr.depth_list(oracle, vr, which):
        out.setdefault(s, (s, scene, []))[2].append((n, i, f, opacity))
    return list(out.values())


def load_scene(gpu, scene, preintegration_first=False):
    """the scene's layout, addressing, transfer function and volume; the pre-integration is switched on before or after the last two"""
    gpu.set_layout(scene.layout)
    gpu.set_wide_addressing(scene.wide)
    if preintegration_first:
        gpu.set_preintegration()
    load(gpu, scene.vox, scene.tf, scene.esl, WINDOW)
    gpu.set_preintegration()


def describe(scene, i, f):
    return (scene.describe(), "layout", scene.layout, "wide", scene.wide, "frame", i, "persp", f.p.view.perspective, (f.p.view.width, f.p.view.height))


def six_comparisons(gpu, ref, what, scene, f, p, opacity, device=False):
    """Both classifications (slab first: the state the scene was loaded in) x the three modes under the frame's clip: the host entry point
    with all three buffers, and with `device` the device entry point with value / alpha NULL in turn.  Returns (frames launched, surface pixels)."""
    import torch
    set_clip(gpu, f.clip)
    frames = surfaces = 0
    for cmode in (SLAB, POINT):
        classify(gpu, cmode)
        for m, mode in enumerate(MODES):
            want = check(gpu, ref, what, scene.vox, p, scene.tf, scene.esl, opacity, mode, cmode, f.clip)
            frames, surfaces = frames + 1, surfaces + int(want.surface.sum())
            if device:
                bufs = [torch.full((p.out_rows, p.out_width), 123.0, dtype=torch.float32, device="cuda") for _ in range(3)]
                torch.cuda.synchronize()                # (the fills run on torch's stream, the frame on the context's)
                with_value = (m + cmode) % 2 == 0
                gpu.render_depth_device(p, opacity, mode, bufs[0].data_ptr(), bufs[1].data_ptr() if with_value else None, None if with_value else bufs[2].data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = [b.cpu().numpy() for b in bufs]
                untouched = np.full_like(got[0], 123.0)
                wrong = (depth_diff(got[0], want.depth), depth_diff(got[1], want.value if with_value else untouched), depth_diff(got[2], untouched if with_value else want.alpha))
                assert wrong == (0, 0, 0) and depth_launch(gpu.last_launch()), (what, "device", opacity, mode, cmode, with_value, wrong, gpu.last_launch())
                frames += 1
    gpu.clear_clip()
    return frames, surfaces


def test_random_scenes_equal_the_restatement(vr, gpu, oracle):
    """14 random scenes x 4 frames, layout and wide addressing alternating per scene, the pre-integration switched on before (odd scenes) or
    after (even scenes) the transfer function and the volume: per frame under its clip, both classifications x the three modes at the
    frame's opacity — depth, value and alpha bits through the host entry point, and on every second frame through the device entry point
    with the value or the alpha buffer NULL; every launch is counted once"""
    ref = DepthRef.instance()
    frames = launched = surfaces = inside = axis = 0
    start = gpu.depth_frames()
    for s, scene, listed in scenes_of(oracle, vr, "random"):
        load_scene(gpu, scene, preintegration_first=s % 2 == 1)
        for n, i, f, opacity in listed:
            k, px = six_comparisons(gpu, ref, describe(scene, i, f), scene, f, f.p, opacity, device=n % 2 == 1)
            frames, launched, surfaces = frames + 1, launched + k, surfaces + px
            inside += int(f.camera_inside())
            axis += int(f.axis_aligned())
    print(f"{frames} random frames, {launched} depth frames launched, {surfaces} surface pixels compared; {inside} cameras inside, {axis} along an axis")
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE and launched == 6 * frames + 6 * (frames // 2) and gpu.depth_frames() == start + launched
    assert surfaces > 0 and inside >= 4 and axis >= 4, (surfaces, inside, axis)          # (tests/test_depth_random_model.py holds the frames to their caps)


def test_holed_scenes_equal_the_restatement(vr, gpu, oracle):
    """The holed scenes — a slab of exact zeros through a random volume under a transfer function with leading zeros, frames of 16 pixels or
    more a side: whole waves skip their samples inside the hole, and under slab classification the first sample behind it needs the
    coordinate of its skipped predecessor.  The six comparisons per frame as drawn, and again with esl = 0 and ray_threshold = 1.0: there
    the march, not the leaping, meets the zero slab on every ray."""
    ref = DepthRef.instance()
    frames = surfaces = 0
    for s, scene, listed in scenes_of(oracle, vr, "holed"):
        load_scene(gpu, scene, preintegration_first=s % 2 == 1)
        for n, i, f, opacity in listed:
            for p in (f.p, fr.full_march(f.p)):
                k, px = six_comparisons(gpu, ref, describe(scene, i, f) + (("full march",) if p is not f.p else ()), scene, f, p, opacity)
                frames, surfaces = frames + k, surfaces + px
    print(f"holed scenes: {frames} depth frames, {surfaces} surface pixels compared")
    assert frames == 2 * 6 * fr.HOLED_SCENES * fr.HOLED_FRAMES and surfaces > 0


@pytest.mark.parametrize("which", LISTS)
def test_edge_opacities(vr, gpu, oracle, which):
    """FIRST at the edges of (0, 1] — the smallest subnormal, the smallest normal, 1, and where the frame terminates early its ray_threshold
    and the next float32 above it — on every frame of the list, both classifications: depth and alpha bits, and the depth bits again
    without the alpha buffer (the ray may stop at its surface).  At the subnormal and the smallest normal opacity the device's own FIRST
    frame has a surface exactly where its own PEAK frame has one: `acc >= opacity` is a compare against a subnormal and the device keeps it."""
    ref = DepthRef.instance()
    frames = surfaces = 0
    for s, scene, listed in scenes_of(oracle, vr, which):
        load_scene(gpu, scene)
        for n, i, f, own in listed:
            what = describe(scene, i, f)
            set_clip(gpu, f.clip)
            for cmode in (SLAB, POINT):
                classify(gpu, cmode)
                peak = gpu.render_depth(f.p, own, "peak")
                for label, opacity in fr.edge_opacities(f.p):
                    want = ref.render(f.p, scene.vox, scene.tf, scene.esl, opacity, "first", cmode, f.clip)
                    depth, alpha = gpu.render_depth(f.p, opacity, "first", alpha=True)
                    alone = gpu.render_depth(f.p, opacity, "first")
                    wrong = depth_diff(depth, want.depth), depth_diff(alpha, want.alpha), depth_diff(alone, want.depth)
                    assert wrong == (0, 0, 0), (what, cmode, label, opacity, wrong, gpu.last_launch())
                    if label in ("subnormal", "tiny"):
                        assert np.array_equal(depth >= 0.0, peak >= 0.0), (what, cmode, label, int(((depth >= 0.0) != (peak >= 0.0)).sum()))
                    frames, surfaces = frames + 1, surfaces + int(want.surface.sum())
            gpu.clear_clip()
    print(f"{which}: {frames} FIRST frames at the edge opacities, {surfaces} surface pixels compared")
    assert frames >= 2 * 3 * len(fr.depth_list(oracle, vr, which)) and surfaces > 0


@pytest.mark.parametrize("which", LISTS)
def test_alpha_is_the_composite_frames_alpha_byte_on_the_device(vr, gpu, oracle, which):
    """Per frame of the list under its clip, with the frame's lighting and shadow set, pre-integration on and off: the alpha byte of the
    composite frame is map_float_int of the depth frame's alpha under the same clip and classification, and the depth frame's three
    buffers keep the restatement's bits: the shadow and the lighting change none"""
    ref = DepthRef.instance()
    compared = 0
    for s, scene, listed in scenes_of(oracle, vr, which):
        load_scene(gpu, scene)
        for n, i, f, opacity in listed:
            what = describe(scene, i, f)
            set_clip(gpu, f.clip)
            gpu.set_lighting(*f.lighting)
            gpu.set_shadow(f.light, f.S, f.shadow_step, f.strength, CUTOFF, f.shadow_sampling)
            for cmode in (SLAB, POINT):
                classify(gpu, cmode)
                frame = gpu.render_volume(f.p)
                assert gpu.last_launch()["shadowed"] == 1, (what, gpu.last_launch())
                want = check(gpu, ref, what, scene.vox, f.p, scene.tf, scene.esl, opacity, MODES[(n + cmode) % 3], cmode, f.clip)
                byte = alpha_byte(want.alpha)
                assert np.array_equal(frame[..., 3], byte), (what, cmode, int((frame[..., 3] != byte).sum()))
                compared += int((byte != 0).sum())
            gpu.clear_shadow()
            gpu.clear_lighting()
            gpu.clear_clip()
    print(f"{which}: {compared} non-zero alpha bytes compared")
    assert compared > 1000, compared


@pytest.mark.parametrize("which", LISTS)
def test_picks(vr, gpu, oracle, which):
    """Picks under the frame's clip, the classification alternating and the modes rotating per frame: every pixel of the random frames of
    at most 256 pixels in one call, the four corners and 60 drawn pixels of the others and of the holed frames.  hit, k, value and alpha
    equal what the whole frame stores at that pixel; position and voxel bits equal the restatement's; a miss is -1 / -1 with zero position
    and voxel; one depth frame is counted per query; the crop and band fields of the params are ignored."""
    ref = DepthRef.instance()
    picks = fr.depth_draws(oracle, vr)["picks"]
    hits = surface_misses = cube_misses = whole = 0
    for s, scene, listed in scenes_of(oracle, vr, which):
        load_scene(gpu, scene)
        for n, i, f, opacity in listed:
            cmode, mode = fr.pick_state(n)
            pixels = picks[which, n]
            set_clip(gpu, f.clip)
            classify(gpu, cmode)
            want = ref.render(f.p, scene.vox, scene.tf, scene.esl, opacity, mode, cmode, f.clip)
            frame = gpu.render_depth(f.p, opacity, mode, value=True, alpha=True)
            before = gpu.depth_frames()
            other = f.p.copy()
            other.x0, other.out_width, other.band_rows, other.band_stride, other.band_first = 5, 7, 3, 2, 1
            got = gpu.pick(other, pixels, opacity, mode)
            assert gpu.depth_frames() == before + len(pixels) and len(got) == len(pixels), (describe(scene, i, f), len(pixels))
            for (x, y), g in zip(pixels, got):
                stored = tuple(float(a[y, x]) for a in frame)
                what = (describe(scene, i, f), cmode, mode, x, y, g, stored)
                assert g["hit"] == (stored[0] >= 0.0) == bool(want.surface[y, x]), what
                one = np.array([g["k"], g["value"], g["alpha"]], np.float32), np.array(g["position"] + g["voxel"], np.float32)
                assert depth_diff(one[0], np.array(stored, np.float32)) == 0 and depth_diff(one[1], want.pick[y, x]) == 0, what
                if not g["hit"]:
                    assert (g["k"], g["value"]) == (-1.0, -1.0) and not any(g["position"]) and not any(g["voxel"]), what
                hits, surface_misses, cube_misses = hits + int(g["hit"]), surface_misses + int(bool(want.rays[y, x]) and not g["hit"]), cube_misses + int(not want.rays[y, x])
            whole += int(len(pixels) == f.p.view.width * f.p.view.height)
            gpu.clear_clip()
    print(f"{which}: {hits} hits, {surface_misses} rays without a surface, {cube_misses} rays that miss the cube; {whole} frames picked whole")
    assert min(hits, surface_misses, cube_misses) > 0 and (which != "random" or whole >= 6), (hits, surface_misses, cube_misses, whole)


def test_first_depth_as_a_backdrop_layer(vr, gpu, oracle):
    """On the random frames whose FIRST frame has a surface, under the frame's clip and each classification: the FIRST depth buffer with an
    opaque colour layer, fed to render_backdrop, gives the frame backdrop_render gives with the restatement's depth"""
    ref, backdrop = DepthRef.instance(), BackdropRef.instance()
    frames = differ = 0
    for s, scene, listed in scenes_of(oracle, vr, "random"):
        load_scene(gpu, scene)
        for n, i, f, opacity in listed:
            what = describe(scene, i, f)
            set_clip(gpu, f.clip)
            for cmode in (SLAB, POINT):
                if not ref.render(f.p, scene.vox, scene.tf, scene.esl, opacity, "first", cmode, f.clip).surface.any():
                    continue
                classify(gpu, cmode)
                want = check(gpu, ref, what, scene.vox, f.p, scene.tf, scene.esl, opacity, "first", cmode, f.clip)
                depth = gpu.render_depth(f.p, opacity, "first")
                layer = np.empty((f.p.out_rows, f.p.out_width, 4), np.uint8)
                layer[...] = (40, 90, 200, 255)
                out = gpu.render_backdrop(f.p, layer, depth)
                expected = backdrop.render(f.p, scene.vox, scene.tf, scene.esl, layer, np.array(want.depth), cmode, f.clip)
                assert diff(out, expected) == 0, (what, cmode, diff(out, expected), gpu.last_launch())
                frames, differ = frames + 1, differ + int(diff(out, backdrop.render(f.p, scene.vox, scene.tf, scene.esl, None, None, cmode, f.clip)) > 0)
            gpu.clear_clip()
    print(f"{frames} backdrop frames over a FIRST depth; {differ} differ from the frame without a layer")
    assert frames >= fr.SCENES * fr.FRAMES_PER_SCENE and 2 * differ >= frames, (frames, differ)     # (at least half of the frames have a surface, per classification)


def test_partitioned_frames(vr, gpu, oracle):
    """Four random frames of at least 8 x 8 pixels with a surface, one mode each, both classifications: every rank of an interleaved band
    partition (2 or 3 ranks, bands of 1, 3 or 16 rows) holds the matching rows of the whole frame's three buffers and -1 / -1 / 0 past
    its end, and a crop in x its columns"""
    ref = DepthRef.instance()
    frames = fr.depth_list(oracle, vr, "random")
    checked = 0
    for n, mode, world, band_rows, x0, cw in fr.depth_draws(oracle, vr)["partitions"]:
        _, s, i, scene, f, opacity = frames[n]
        assert f.p.view.width >= 8 and f.p.view.height >= 8
        load_scene(gpu, scene)
        set_clip(gpu, f.clip)
        for cmode in (SLAB, POINT):
            classify(gpu, cmode)
            want = ref.render(f.p, scene.vox, scene.tf, scene.esl, opacity, mode, cmode, f.clip)
            assert want.surface.any()
            whole = (want.depth, -1), (want.value, -1), (want.alpha, 0)
            for rank in range(world):
                p, per_rank = vr.band_partition(f.p.copy(), rank, world, band_rows)
                rows = per_rank * band_rows
                got = gpu.render_depth(p, opacity, mode, value=True, alpha=True)
                for buffer, (full, beyond) in zip(got, whole):
                    assert buffer.shape == (rows, f.p.view.width) and depth_diff(buffer, expected_bands(full, rank, world, band_rows, rows, beyond=beyond)) == 0, \
                        (describe(scene, i, f), mode, cmode, world, band_rows, rank)
                checked += 1
            crop = f.p.copy()
            crop.x0, crop.out_width = x0, cw
            got = gpu.render_depth(crop, opacity, mode, value=True, alpha=True)
            for buffer, (full, beyond) in zip(got, whole):
                assert depth_diff(buffer, full[:, x0:x0 + cw]) == 0, (describe(scene, i, f), mode, cmode, "crop", x0, cw)
            checked += 1
        gpu.clear_clip()
    assert checked >= 4 * 2 * 3


@needs_bounds_lib
def test_under_the_bounds_checked_build():
    """The random scenes, the holed scenes and the picks once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py):
    every gather address is held against its array — a violation fails the frame (VrError) — and the bits still equal the restatement"""
    run_under_bounds_build(__file__, "random_scenes or holed_scenes or picks", 4, timeout=900)
