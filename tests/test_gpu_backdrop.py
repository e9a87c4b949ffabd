"""GPU tier of the backdrop and hybrid frames (vr_hip_render_backdrop* / vr_hip_render_hybrid*): every frame the four composite_backdrop*
kernel families render is held byte for byte against backdrop_render / hybrid_render of tests/feature_ref.c, the contract of
include/vr_hip.h restated with the CPU oracle's statics — no tolerance anywhere.  tests/test_backdrop_model.py ties that restatement to the pinned composites and shows that the frames
compared here tell three wrong readings of the contract apart."""
import ctypes as C

import numpy as np
import pytest

from backdrop_helpers import BACKDROP_VOLUMES, HYBRID_LEVELS, BackdropRef, synthetic_layer, tier_frames
from clip_helpers import CLIPS, set_clip
from feature_random import EDGE_DTYPES, EDGE_SHAPES, edge_scene
from gpu_feature import PATH_VOLUMES, diff, expected_bands, load, needs_bounds_lib, reset_context, run_driver, run_under_bounds_build, sweep_paths
from iso_helpers import IsoRef, depth_bits, frame_params
from light_helpers import LIGHTINGS, PHONG
from light_helpers import lit_views as backdrop_views
from light_helpers import lit_volumes as backdrop_volumes
from mip_helpers import MipRef
from shadow_helpers import FRAME_SCENES, LIGHTS, ShadowRef
from slab_helpers import POINT, SLAB
from slab_helpers import slab_scene as backdrop_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return backdrop_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state or a forced path behind.  (Setting the layout drops the brick
    copies; every test that renders through the shared context begins with load or set_volume, which drops them anyway.)"""
    yield
    reset_context(vr, gpu)


def backdrop_launch(gpu, info):
    """what every backdrop frame's launch looks like: what a clipped frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", BACKDROP_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """Synthetic layers from the seeded generator (random colour words; depths -1, NaN, 0, +inf, before kx, inside the segment, beyond ky
    and exactly on a sample, mixed per pixel): nine views x {default mode, full march, early termination alone} x {the ray step, four
    times it: the clamping variant} x {cue-lit, light_kd = 0} — the restatement's bytes, on the backdrop kernels, one more frame counted each"""
    ref = BackdropRef.instance()
    loaded = False
    frames = shown = 0
    for what, vox, p, tf, esl, rgba, depth in tier_frames(vr, golden, oracle, volumes, name, sampling):
        if not loaded:
            load(gpu, vox, tf, esl)
            loaded = True
        before = gpu.backdrop_frames()
        out = gpu.render_backdrop(p, rgba, depth)
        info = gpu.last_launch()
        want = ref.render(p, vox, tf, esl, rgba, depth)
        assert diff(out, want) == 0, (what, diff(out, want), info)
        assert backdrop_launch(gpu, info) and info["shadowed"] == 0 and gpu.backdrop_frames() == before + 1, info
        frames, shown = frames + 1, shown + int(ref.render(p, vox, tf, esl).any(axis=-1).sum())
    print(f"{name} sampling {sampling}: {frames} frames, {shown} pixels with volume in them compared")
    assert frames == 108 and shown > 108 * 300, (frames, shown)


@pytest.mark.parametrize("dtype", EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65) from views 0, 1 and 5 under both clips of its frames: the
    cue-lit backdrop frame, and the pre-integrated one under the lighting and the light grid of those frames"""
    ref, shadow_ref = BackdropRef.instance(), ShadowRef.instance()
    gpu.set_window_buffer(64, 64)
    for i, shape in enumerate(EDGE_SHAPES):
        s = edge_scene(oracle, vr, shape, dtype)
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        for j, f in enumerate(s.frames):
            rgba, depth = synthetic_layer(ref, f.p, s.vox, s.tf, s.esl, f.clip, salt=100 + 8 * i + j)
            set_clip(gpu, f.clip)
            gpu.clear_lighting()
            gpu.clear_shadow()
            gpu.clear_preintegration()
            out = gpu.render_backdrop(f.p, rgba, depth)
            want = ref.render(f.p, s.vox, s.tf, s.esl, rgba, depth, POINT, f.clip)
            assert diff(out, want) == 0, (shape, dtype, f.view, f.clip_name, "cue", diff(out, want), gpu.last_launch())
            q = shadow_ref.build(f.light, f.S, f.shadow_step, s.vox, s.tf, sampling=f.shadow_sampling, clip=f.clip)
            gpu.set_lighting(*f.lighting)
            gpu.set_shadow(f.light, f.S, float(f.shadow_step), f.strength, sampling=f.shadow_sampling)
            gpu.set_preintegration()
            out = gpu.render_backdrop(f.p, rgba, depth)
            want = ref.render(f.p, s.vox, s.tf, s.esl, rgba, depth, SLAB, f.clip, f.lighting, q, f.strength)
            assert diff(out, want) == 0, (shape, dtype, f.view, f.clip_name, "slab, lit and shadowed", diff(out, want), gpu.last_launch())


def test_every_path_agrees(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9 (3, 4, 6, 7, 8 fall back), wide addressing 0 / 1 / 2 / +4,
    every lane order x wave shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, never a run copy or a column window,
    never a measured order; u8 and u16 (oct bricks); the cue-lit family and, under a lighting, the lit one"""
    ref = BackdropRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in backdrop_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for k, (label, view) in enumerate(views):
            for sampling, full_march in ((1, True), (2, False)):
                vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
                rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=200 + 2 * k + sampling)
                cases.append((label, sampling, p, rgba, depth, ref.render(p, vox, tf, esl, rgba, depth), ref.render(p, vox, tf, esl, rgba, depth, lighting=PHONG)))
        load(gpu, vox, tf, esl)
        seen = set()

        def check(what):
            for label, sampling, p, rgba, depth, want, want_lit in cases:
                for lighting, expected in ((None, want), (PHONG, want_lit)):
                    if lighting is None:
                        gpu.clear_lighting()
                    else:
                        gpu.set_lighting(*lighting)
                    out = gpu.render_backdrop(p, rgba, depth)
                    info = gpu.last_launch()
                    assert diff(out, expected) == 0, (name, what, label, sampling, lighting, diff(out, expected), info)
                    assert backdrop_launch(gpu, info), (name, what, label, sampling, info)
                    seen.add(info["layout"])
        sweep_paths(vr, gpu, check)
        assert seen == expect, (name, seen)


def test_bands_crop_and_in_place(vr, gpu, golden, oracle, volumes):
    """The layers are partitioned like the output.  Interleaved bands of 3 rows with stride 2, both band_first (72 rows: the last band of
    the second rank lies beyond the view, where every ray is a miss and a pixel with a surface is the layer's colour word) and a crop in x
    equal the matching rows / columns of the whole frame; the device entry point renders out of place and, with the output on the colour
    layer, in place, in one launch each, and leaves the layer alone when it is not the output"""
    import torch
    name = "blob_40x24x56"
    ref = BackdropRef.instance()
    vox, whole, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 70, 5), 1, False)
    load(gpu, vox, tf, esl)
    rgba, depth = synthetic_layer(ref, whole, vox, tf, esl, salt=300)
    want = ref.render(whole, vox, tf, esl, rgba, depth)
    assert diff(want, rgba) > 1000 and diff(want, ref.render(whole, vox, tf, esl)) > 1000
    rng = np.random.default_rng(5)
    for first in (0, 1):
        p, per_rank = vr.band_partition(whole.copy(), first, 2, 3)
        rows = per_rank * 3
        assert p.out_rows == rows == 36
        gy = np.array([((ly // 3) * 2 + first) * 3 + ly % 3 for ly in range(rows)])
        inside = gy < 70
        assert inside.all() == (first == 0)
        band_rgba = rng.integers(0, 256, size=(rows, 120, 4), dtype=np.uint8)
        band_depth = np.where(rng.random(size=(rows, 120)) < 0.5, np.float32(1.5), np.float32(np.nan)).astype(np.float32)
        band_rgba[inside], band_depth[inside] = rgba[gy[inside]], depth[gy[inside]]
        expected = expected_bands(want, first, 2, 3, rows)
        beyond = ~inside[:, None] & (band_depth >= 0)
        expected[beyond] = band_rgba[beyond]
        out = gpu.render_backdrop(p, band_rgba, band_depth)
        assert np.array_equal(out, expected), (first, diff(out, expected))
    crop = whole.copy()
    crop.x0, crop.out_width = 24, 40
    assert np.array_equal(gpu.render_backdrop(crop, rgba[:, 24:64], depth[:, 24:64]), want[:, 24:64])
    layer = torch.from_numpy(np.array(rgba)).cuda()
    dlayer = torch.from_numpy(np.array(depth)).cuda()
    buf = torch.full((70, 120, 4), 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                            # (the uploads and the fill run on torch's stream, the frame on the context's)
    gpu.timing_reset()
    before = gpu.backdrop_frames()
    gpu.render_backdrop_device(whole, layer.data_ptr(), dlayer.data_ptr(), buf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and gpu.backdrop_frames() == before + 1
    assert diff(buf.cpu().numpy(), want) == 0 and np.array_equal(layer.cpu().numpy(), rgba)
    gpu.render_backdrop_device(whole, layer.data_ptr(), dlayer.data_ptr(), layer.data_ptr(), stream)
    torch.cuda.synchronize()
    assert diff(layer.cpu().numpy(), want) == 0 and np.array_equal(depth_bits(dlayer.cpu().numpy()), depth_bits(depth))


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
def test_backdrop_with_clip(vr, gpu, golden, oracle, volumes, clip_name):
    """The backdrop kernels run clip_segment: under each of CLIPS the frames equal the restatement (the layer's depths are placed on the
    clipped segments) and differ from the unclipped ones"""
    name, clip = "bucky", CLIPS[clip_name]
    ref = BackdropRef.instance()
    for i, (label, view) in enumerate(backdrop_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if i == 0 and sampling == 1:
                load(gpu, vox, tf, esl)
                set_clip(gpu, clip)
            rgba, depth = synthetic_layer(ref, p, vox, tf, esl, clip, salt=400 + 2 * i + sampling)
            out = gpu.render_backdrop(p, rgba, depth)
            want = ref.render(p, vox, tf, esl, rgba, depth, clip=clip)
            assert diff(out, want) == 0 and backdrop_launch(gpu, gpu.last_launch()), (clip_name, label, sampling, full_march, diff(out, want))
    assert diff(want, ref.render(p, vox, tf, esl, rgba, depth)) > 0


@pytest.mark.parametrize("name", sorted(FRAME_SCENES))
def test_backdrop_with_shadow(vr, gpu, golden, oracle, volumes, name):
    """The base family takes the shadow as a kernel argument: with the light grids of the shadow tests at strength 1, 0.6 and 0 the frames
    equal the restatement (shadowed == 1, on the backdrop kernels); strength 0 gives the bytes of the backdrop frame without a shadow; the
    grid is built once"""
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = BackdropRef.instance(), ShadowRef.instance()
    q = None
    for i, (label, view) in enumerate(backdrop_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if q is None:
                load(gpu, vox, tf, esl)
                q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
            rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=500 + 2 * i + sampling)
            for strength in (1.0, 0.6, 0.0):
                gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), strength)
                before = gpu.backdrop_frames()
                out = gpu.render_backdrop(p, rgba, depth)
                info = gpu.last_launch()
                want = ref.render(p, vox, tf, esl, rgba, depth, q=q, strength=strength)
                assert diff(out, want) == 0, (name, label, sampling, full_march, strength, diff(out, want), info)
                assert info["shadowed"] == 1 and backdrop_launch(gpu, info) and gpu.backdrop_frames() == before + 1, info
            assert diff(want, ref.render(p, vox, tf, esl, rgba, depth)) == 0            # strength 0
    vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, backdrop_views(vr, golden, name)[1][1], 1, False)
    rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=503)
    assert diff(ref.render(p, vox, tf, esl, rgba, depth, q=q, strength=1.0), ref.render(p, vox, tf, esl, rgba, depth)) > 0


@pytest.mark.parametrize("name", ("bucky", "plateau", "random_u16"))
def test_backdrop_with_lighting_and_preintegration(vr, gpu, golden, oracle, volumes, name):
    """composite_backdrop_lit, composite_backdrop_slab and composite_backdrop_slab_lit: each of LIGHTINGS, the pre-integration alone, and
    both, give the restatement's bytes; the backdrop counter moves once per frame, the lighting's and the pre-integration's with it"""
    ref = BackdropRef.instance()
    loaded = False
    for i, (label, view) in enumerate(backdrop_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not loaded:
                load(gpu, vox, tf, esl)
                loaded = True
            rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=600 + 2 * i + sampling)
            for mode in (POINT, SLAB):
                gpu.set_preintegration(mode == SLAB)
                for lighting in (LIGHTINGS if mode == POINT else (None, PHONG)):
                    if lighting is None:
                        gpu.clear_lighting()
                    else:
                        gpu.set_lighting(*lighting)
                    before = gpu.backdrop_frames(), gpu.lighting_frames(), gpu.preint_frames()
                    out = gpu.render_backdrop(p, rgba, depth)
                    info = gpu.last_launch()
                    want = ref.render(p, vox, tf, esl, rgba, depth, mode, lighting=lighting)
                    assert diff(out, want) == 0, (name, label, sampling, full_march, mode, lighting, diff(out, want), info)
                    after = gpu.backdrop_frames(), gpu.lighting_frames(), gpu.preint_frames()
                    assert backdrop_launch(gpu, info) and after == (before[0] + 1, before[1] + int(lighting is not None), before[2] + int(mode == SLAB)), (before, after)


def test_all_four_states_together(vr, gpu, golden, oracle, volumes):
    """Clip `both`, the top light's grid (built under that clip) at strength 0.6, and every combination of lighting and pre-integration:
    the four families, each counted"""
    name, clip = "bucky", CLIPS["both"]
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = BackdropRef.instance(), ShadowRef.instance()
    q = None
    start = gpu.backdrop_frames()
    frames = 0
    for i, (label, view) in enumerate(backdrop_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if q is None:
                load(gpu, vox, tf, esl)
                set_clip(gpu, clip)
                q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf, clip=clip)
                gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), 0.6)
            rgba, depth = synthetic_layer(ref, p, vox, tf, esl, clip, salt=700 + 2 * i + sampling)
            for mode in (POINT, SLAB):
                gpu.set_preintegration(mode == SLAB)
                for lighting in (None, PHONG):
                    if lighting is None:
                        gpu.clear_lighting()
                    else:
                        gpu.set_lighting(*lighting)
                    out = gpu.render_backdrop(p, rgba, depth)
                    want = ref.render(p, vox, tf, esl, rgba, depth, mode, clip, lighting, q, 0.6)
                    assert diff(out, want) == 0, (label, sampling, full_march, mode, lighting, diff(out, want), gpu.last_launch())
                    frames += 1
    assert want.any() and gpu.backdrop_frames() == start + frames == start + 72


@pytest.mark.parametrize("name", BACKDROP_VOLUMES)
def test_hybrid_equals_the_restatement(vr, gpu, golden, oracle, volumes, name):
    """The hybrid at the volume's level of HYBRID_LEVELS, refine 0 and 4: vr_hip_render_hybrid_device equals render_iso_device followed by
    render_backdrop_device in place on the GPU, and hybrid_render's frame and depth bits, with the depth buffer given and NULL; so do the
    host entry points.  Default mode and full march: with esl on the isosurface frame skips fetches and the depth is the same, bit for bit."""
    import torch
    ref = BackdropRef.instance()
    level = HYBRID_LEVELS[name]
    stream = torch.cuda.current_stream().cuda_stream
    loaded = False
    for label, view in backdrop_views(vr, golden, name):
        depths = {}
        for sampling, full_march in ((1, False), (1, True), (2, False)):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not loaded:
                load(gpu, vox, tf, esl)
                loaded = True
            shape = (p.out_rows, p.out_width)
            for refine in (0, 4):
                want, want_depth, want_iso = ref.hybrid(p, vox, tf, esl, level, refine)
                two = torch.full(shape + (4,), 77, dtype=torch.uint8, device="cuda")
                two_depth = torch.full(shape, 123.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()                # (the fills run on torch's stream, the frame on the context's)
                gpu.render_iso_device(p, level, refine, two.data_ptr(), two_depth.data_ptr(), stream)
                gpu.render_backdrop_device(p, two.data_ptr(), two_depth.data_ptr(), two.data_ptr(), stream)
                one = torch.full(shape + (4,), 78, dtype=torch.uint8, device="cuda")
                one_depth = torch.full(shape, 124.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()                # (the fills run on torch's stream, the frame on the context's)
                before = gpu.backdrop_frames()
                gpu.render_hybrid_device(p, level, refine, one.data_ptr(), one_depth.data_ptr(), stream)
                own = torch.full(shape + (4,), 79, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()                # (the fill runs on torch's stream, the frame on the context's)
                gpu.render_hybrid_device(p, level, refine, own.data_ptr(), None, stream)
                torch.cuda.synchronize()
                what = (name, label, sampling, full_march, refine)
                assert gpu.backdrop_frames() == before + 2 and backdrop_launch(gpu, gpu.last_launch()), what
                assert torch.equal(one, two) and torch.equal(one_depth.view(torch.int32), two_depth.view(torch.int32)) and torch.equal(own, one), what
                assert diff(one.cpu().numpy(), want) == 0 and np.array_equal(depth_bits(one_depth.cpu().numpy()), depth_bits(want_depth)), what
                host, host_depth = gpu.render_hybrid(p, level, refine, depth=True)
                assert diff(host, want) == 0 and np.array_equal(depth_bits(host_depth), depth_bits(want_depth)), what
                assert np.array_equal(gpu.render_hybrid(p, level, refine), host), what
                if sampling == 1:
                    depths[(full_march, refine)] = depth_bits(want_depth)
        for refine in (0, 4):
            assert np.array_equal(depths[(False, refine)], depths[(True, refine)])


def test_hybrid_with_every_state(vr, gpu, golden, oracle, volumes):
    """The isosurface frame of a hybrid sees the clip and ignores shadow, lighting and pre-integration; the composite pass sees all four"""
    name, clip = "bucky", CLIPS["both"]
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = BackdropRef.instance(), ShadowRef.instance()
    q = None
    for label, view in backdrop_views(vr, golden, name):
        vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 1, False)
        if q is None:
            load(gpu, vox, tf, esl)
            set_clip(gpu, clip)
            q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf, clip=clip)
            gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), 0.6)
            gpu.set_lighting(*PHONG)
            gpu.set_preintegration()
        out, depth = gpu.render_hybrid(p, HYBRID_LEVELS[name], 4, depth=True)
        want, want_depth, want_iso = ref.hybrid(p, vox, tf, esl, HYBRID_LEVELS[name], 4, SLAB, clip, PHONG, q, 0.6)
        assert diff(out, want) == 0 and np.array_equal(depth_bits(depth), depth_bits(want_depth)), (label, diff(out, want))
        assert diff(gpu.render_iso(p, HYBRID_LEVELS[name], 4), want_iso) == 0, label
    assert diff(want, want_iso) > 0


def test_state_off_is_untouched(vr, gpu, golden, oracle, volumes):
    """A backdrop is an argument, not state.  A plain default-mode frame (256 x 256: 128 tiles, under the measured-cost tile order) after
    backdrop and hybrid frames equals the frame before them and still starts its tiles in the recorded order; the backdrop frames start
    theirs in grid order; the counters of the lighting and the pre-integration do not move, and a shadow's light grid is not rebuilt"""
    ref = BackdropRef.instance()
    vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    want_plain = ref.render(p, vox, tf, esl)
    for k in range(3):
        first = gpu.render_volume(p)
    assert diff(first, want_plain) == 0 and gpu.last_launch()["ordered"] == 1
    rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=800)
    counters = gpu.lighting_frames(), gpu.preint_frames(), gpu.shadow_builds()[0]
    count = gpu.backdrop_frames()
    for k in range(3):
        assert diff(gpu.render_backdrop(p, rgba, depth), ref.render(p, vox, tf, esl, rgba, depth)) == 0
        assert gpu.last_launch()["ordered"] == 0
    assert diff(gpu.render_hybrid(p, HYBRID_LEVELS["bucky"], 4), ref.hybrid(p, vox, tf, esl, HYBRID_LEVELS["bucky"], 4)[0]) == 0
    assert gpu.backdrop_frames() == count + 4
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["ordered"] == 1 and gpu.backdrop_frames() == count + 4
    assert (gpu.lighting_frames(), gpu.preint_frames(), gpu.shadow_builds()[0]) == counters
    gpu.set_shadow(LIGHTS["top"], 17, float(p.ray_step), 1.0)
    shadowed = gpu.render_volume(p)
    builds = gpu.shadow_builds()[0]
    assert builds == counters[2] + 1
    gpu.render_backdrop(p, rgba, depth)
    gpu.render_hybrid(p, HYBRID_LEVELS["bucky"], 4)
    assert np.array_equal(gpu.render_volume(p), shadowed) and gpu.shadow_builds()[0] == builds


def test_errors_and_what_ignores_it(vr, gpu, golden, oracle, volumes):
    """NEAREST is refused, NULL structs and NULL members are refused (VR_ERR_INVALID), nothing is counted; MIP and isosurface frames equal
    their restatements afterwards"""
    import torch
    ref = BackdropRef.instance()
    vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 3), 1, False)
    load(gpu, vox, tf, esl)
    rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=900)
    assert diff(gpu.render_backdrop(p, rgba, depth), ref.render(p, vox, tf, esl, rgba, depth)) == 0
    count = gpu.backdrop_frames()
    nearest = p.copy()
    nearest.sampling = 0
    with pytest.raises(vr.VrError) as e:
        gpu.render_backdrop(nearest, rgba, depth)
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    with pytest.raises(vr.VrError) as e:
        gpu.render_hybrid(nearest, 100.0, 4)
    assert e.value.code == 1
    L = vr.lib()
    buf = torch.zeros((80, 80, 4), dtype=torch.uint8, device="cuda")
    dbuf = torch.zeros((80, 80), dtype=torch.float32, device="cuda")
    host = np.zeros((80, 80, 4), np.uint8)
    iso = vr.VrIso(100.0, 4)
    for layer in (None, vr.VrBackdrop(None, dbuf.data_ptr()), vr.VrBackdrop(buf.data_ptr(), None)):
        arg = None if layer is None else C.byref(layer)
        assert L.vr_hip_render_backdrop_device(gpu._ctx, C.byref(p), arg, buf.data_ptr(), None) == 1
        assert L.vr_hip_render_backdrop(gpu._ctx, C.byref(p), arg, host.ctypes.data) == 1
    both = vr.VrBackdrop(buf.data_ptr(), dbuf.data_ptr())
    assert L.vr_hip_render_backdrop_device(gpu._ctx, C.byref(p), C.byref(both), None, None) == 1
    assert L.vr_hip_render_backdrop_device(gpu._ctx, None, C.byref(both), buf.data_ptr(), None) == 1
    assert L.vr_hip_render_hybrid_device(gpu._ctx, C.byref(p), None, buf.data_ptr(), None, None) == 1
    assert L.vr_hip_render_hybrid_device(gpu._ctx, C.byref(p), C.byref(iso), None, None, None) == 1
    assert L.vr_hip_render_hybrid(gpu._ctx, C.byref(p), C.byref(iso), None, None) == 1
    assert L.vr_hip_backdrop_frames(gpu._ctx, None) == 1
    torch.cuda.synchronize()
    assert gpu.backdrop_frames() == count
    for sampling in (0, 1):
        fp = frame_params(vr, oracle, vox, vr.benchmark_view(80, 80, 3), sampling, 1)
        assert diff(gpu.render_mip(fp), MipRef.instance().render(fp, vox, tf)[0]) == 0
        if sampling:
            out, d = gpu.render_iso(fp, 100.0, 4, depth=True)
            want, want_d, _ = IsoRef.instance().render(fp, vox, tf, 100.0, 4)
            assert diff(out, want) == 0 and np.array_equal(depth_bits(d), depth_bits(want_d))
    assert gpu.backdrop_frames() == count


@needs_bounds_lib
def test_backdrop_frames_under_the_bounds_checked_build():
    """A subset of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every gather address is
    held against its array — a violation fails the frame (VrError) — and the bytes still equal the restatement"""
    run_under_bounds_build(__file__, "edge_shapes or every_path or all_four_states or hybrid_with_every_state or (frames_equal and bucky)", 7, timeout=900)


def test_driver_hybrid_flag(golden, tmp_path):
    """volr_bench -hybrid (HipRenderer::set_hybrid through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance 2,
    256 x 256 — the restatement's frame; with -shadow 17 -phong 0.25 0.65 0.4 4 -preint the composite pass sees all three"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = BackdropRef.instance()
    q = ShadowRef.instance().build(tuple(p.view.light_pos), 17, p.ray_step, vox, st["tf"])
    level = HYBRID_LEVELS["bucky"]
    for extra, mode, lighting, grid in (([], POINT, None, None), (["-shadow", "17", "-phong", "0.25", "0.65", "0.4", "4", "-preint"], SLAB, PHONG, q)):
        out, rgb = run_driver(tmp_path, "-hybrid", str(level), *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Hybrid: isosurface at level" in out.stdout
        want, _, iso = ref.hybrid(p, vox, st["tf"], st["esl"], level, 4, mode, lighting=lighting, q=grid, strength=1.0)
        assert np.array_equal(rgb, want[..., :3]), (extra, int((rgb != want[..., :3]).any(axis=-1).sum()))
        assert diff(want, iso) > 1000 and diff(want, ref.render(p, vox, st["tf"], st["esl"], None, None, mode, lighting=lighting, q=grid)) > 1000
    for bad in (["-mip"], ["-iso", "100"], ["-devices", "0,0"], ["-r", "0"]):
        out, _ = run_driver(tmp_path, *bad, "-hybrid", str(level), size=(128, 128), pose=None, renderer=None if "-r" in bad else "1", output=None)
        assert out.returncode != 0 and "Error: -hybrid" in out.stdout, (bad, out.stdout)
