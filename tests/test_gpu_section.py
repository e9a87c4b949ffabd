"""GPU tier of the section frames (vr_hip_render_section* / vr_hip_render_section_in_volume*): every frame the section_kernel family renders
is held byte for byte — RGBA and depth bits, no tolerance anywhere — against section_render / section_in_volume_render of
tests/section_ref.c, the contract of include/vr_hip.h restated with the CPU oracle's statics.  tests/test_section_model.py ties that
restatement to the clipped MIP and shows that the frames compared here carry sections and tell four wrong readings of the contract apart."""
import ctypes as C

import numpy as np
import pytest

import feature_random as fr
from backdrop_helpers import BackdropRef
from clip_helpers import CLIPS, IDENTITY, set_clip
from gpu_feature import (PATH_VOLUMES, depth_diff, diff, expected_bands, load, needs_bounds_lib, reset_context, run_driver, run_under_bounds_build,
                         sweep_paths)
from iso_helpers import IsoRef, frame_params
from light_helpers import PHONG, lit_views, lit_volumes
from mip_helpers import MipRef
from section_helpers import MODES, SECTION_VOLUMES, WINDOWS, SectionRef, half_width_of, planes_of, tier_frames, unit
from shadow_helpers import FRAME_SCENES, LIGHTS, ShadowRef
from slab_helpers import SLAB, slab_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout or a forced path behind"""
    yield
    reset_context(vr, gpu)


def section_launch(info):
    """what every section frame's launch looks like: what a clipped MIP frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


def check(gpu, ref, what, vox, p, tf, plane, h, mode, window, clip=IDENTITY):
    """the host entry point with depth (RGBA and depth bits) and without (the same RGBA) against section_render; returns the frame"""
    want, want_depth, count, _ = ref.render(p, vox, tf, plane, h, mode, window, clip)
    out, depth = gpu.render_section(p, plane, h, mode, window, depth=True)
    info = gpu.last_launch()
    assert diff(out, want) == 0 and depth_diff(depth, want_depth) == 0, (what, diff(out, want), depth_diff(depth, want_depth), info)
    assert section_launch(info), (what, info)
    assert (depth[depth != -1.0] >= 0.0).all(), (what, "intersect clamps kx at 0: the depth of a hit reads as a surface to a backdrop frame")
    assert np.array_equal(gpu.render_section(p, plane, h, mode, window), out), (what, "the bytes depend on the depth buffer")
    return want, count


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", SECTION_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """Nine views x six sections (facing the view, two diagonal, two across an axis, and the cut: the clip plane on the section) x the four
    modes, transfer-function and grey-window colouring, the ray step and four times it: RGBA and depth bits, depth given and NULL, one
    frame counted each"""
    ref = SectionRef.instance()
    loaded = None
    frames = sections = 0
    start = gpu.section_frames()
    for what, vox, p, tf, plane, h, mode, window, clip in tier_frames(vr, golden, oracle, volumes, name, sampling):
        if loaded is None:
            load(gpu, vox, tf)
        if clip != loaded:
            set_clip(gpu, clip)
            loaded = clip
        want, count = check(gpu, ref, what, vox, p, tf, plane, h, mode, window, clip)
        frames, sections = frames + 1, sections + int(((count != 0xffffffff) & (count > 0)).sum())
    print(f"{name} sampling {sampling}: {frames} frames, {sections} section pixels compared")
    assert frames == 216 and sections > 216 * 300 and gpu.section_frames() == start + 2 * frames, (frames, sections)


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65) from views 0, 1 and 5 at 48 x 40 under both clips of its
    frames (their esl and thresholds, which a section frame ignores): the section facing the view and a diagonal one off the centre, the
    four modes, the colouring alternating"""
    ref = SectionRef.instance()
    gpu.set_window_buffer(*fr.EDGE_SIZE)
    frames = 0
    for i, shape in enumerate(fr.EDGE_SHAPES):
        s = fr.edge_scene(oracle, vr, shape, dtype)
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        window = (10.0, 250.0) if dtype == "uint8" else (2570.0, 64250.0)
        for j, f in enumerate(s.frames):
            set_clip(gpu, f.clip)
            sections = planes_of(f.p.view)
            for k, (label, plane, _) in enumerate((sections[0], sections[2])):
                for m, mode in enumerate(MODES):
                    h = 0.0 if mode == "point" else half_width_of(f.p, "edge")
                    check(gpu, ref, (shape, dtype, f.view, f.clip_name, label, mode), s.vox, f.p, s.tf, plane, h, mode, window if (i + j + k + m) % 2 else None, f.clip)
                    frames += 1
    assert frames == 11 * 6 * 2 * 4


def test_random_scenes_and_frame_sizes(vr, gpu, oracle):
    """The 14 random scenes of tests/feature_random.py x 4 frames (frame sizes from 1 x 1 to 69 x 49, cameras inside the cube, exact zeros
    in the direction, the four-fold step), layout and wide addressing alternating per scene, under each frame's clip: a random plane
    through a random point of the cube per frame, the four modes, the colouring alternating"""
    ref = SectionRef.instance()
    rng = fr.generator(611)
    frames = 0
    for scene in fr.random_scenes(oracle, vr):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
        top = 255.0 if scene.vox.dtype == np.uint8 else 65535.0
        for i, f in enumerate(scene.frames):
            n = unit(rng.normal(size=3))
            plane = n + (float(np.float32(-np.dot(n, rng.uniform(-0.6, 0.6, size=3)))),)
            set_clip(gpu, f.clip)
            for m, mode in enumerate(MODES):
                h = 0.0 if mode == "point" else half_width_of(f.iso, scene.name)
                what = (scene.describe(), "layout", scene.layout, "wide", scene.wide, "frame", i, mode, plane, (f.iso.view.width, f.iso.view.height))
                check(gpu, ref, what, scene.vox, f.iso, scene.tf, plane, h, mode, (0.04 * top, 0.9 * top) if (i + m) % 2 else None, f.clip)
                frames += 1
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE * 4


def test_every_path_agrees(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / 4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes and depth bits, never a run copy or a column window, never a
    measured order; u8 and u16 (oct bricks); a POINT frame coloured by the transfer function and a MEAN frame under the window"""
    ref = SectionRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in lit_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for k, (label, view) in enumerate(views):
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + k % 2, True)
            plane = planes_of(view)[1 + k][1]
            cases.append((label, p, plane, 0.0, "point", None))
            cases.append((label, p, plane, half_width_of(p, name), "mean", WINDOWS[name]))
        load(gpu, vox, tf, esl)
        seen = set()

        def check_all(what):
            for label, p, plane, h, mode, window in cases:
                check(gpu, ref, (name, what, label, mode), vox, p, tf, plane, h, mode, window)
                seen.add(gpu.last_launch()["layout"])
        sweep_paths(vr, gpu, check_all)
        assert seen == expect, (name, seen)


def test_bands_crop_and_device_entry_point(vr, gpu, golden, oracle, volumes):
    """Interleaved bands of 3 rows with stride 2, both band_first (72 rows over a view of 70: the last band of the second rank lies beyond
    the view, where the pixel is the miss word and the depth -1) and a crop in x equal the matching rows / columns of the whole frame,
    RGBA and depth; the device entry point renders the same in one launch, with a depth buffer and without"""
    import torch
    name = "blob_40x24x56"
    ref = SectionRef.instance()
    vox, whole, tf, esl = slab_scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 70, 5), 1, True)
    load(gpu, vox, tf, esl)
    plane, h, window = planes_of(whole.view)[1][1], half_width_of(whole, name), WINDOWS[name]
    for mode in ("point", "mean"):
        hw = 0.0 if mode == "point" else h
        want, want_depth, count, _ = ref.render(whole, vox, tf, plane, hw, mode, window)
        assert (count == 0).sum() > 500 and ((count != 0xffffffff) & (count > 0)).sum() > 1000
        for first in (0, 1):
            p, per_rank = vr.band_partition(whole.copy(), first, 2, 3)
            rows = per_rank * 3
            assert p.out_rows == rows == 36
            expected, expected_depth = expected_bands(want, first, 2, 3, rows), expected_bands(want_depth, first, 2, 3, rows, beyond=-1)
            assert expected_bands(np.ones(70, bool), first, 2, 3, rows).all() == (first == 0)      # (rank 1 holds rows beyond the view)
            out, depth = gpu.render_section(p, plane, hw, mode, window, depth=True)
            assert np.array_equal(out, expected) and depth_diff(depth, expected_depth) == 0, (mode, first, diff(out, expected))
        crop = whole.copy()
        crop.x0, crop.out_width = 24, 40
        out, depth = gpu.render_section(crop, plane, hw, mode, window, depth=True)
        assert np.array_equal(out, want[:, 24:64]) and depth_diff(depth, want_depth[:, 24:64]) == 0
        buf = torch.full((70, 120, 4), 77, dtype=torch.uint8, device="cuda")
        dbuf = torch.full((70, 120), 123.0, dtype=torch.float32, device="cuda")
        alone = torch.full((70, 120, 4), 78, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()                        # (the fills run on torch's stream, the frame on the context's)
        gpu.timing_reset()
        before = gpu.section_frames()
        gpu.render_section_device(whole, plane, hw, mode, window, buf.data_ptr(), dbuf.data_ptr(), stream)
        torch.cuda.synchronize()
        assert gpu.timing().launches == 1 and gpu.section_frames() == before + 1 and section_launch(gpu.last_launch())
        gpu.render_section_device(whole, plane, hw, mode, window, alone.data_ptr(), None, stream)
        torch.cuda.synchronize()
        assert diff(buf.cpu().numpy(), want) == 0 and depth_diff(dbuf.cpu().numpy(), want_depth) == 0 and torch.equal(alone, buf)


def test_params_a_section_ignores(vr, gpu, golden, oracle, volumes):
    """params.esl, ray_threshold, light_kd and light_pos are ignored: with esl on, a threshold of 0.3, no cue and another light the bytes
    and the depth are the same"""
    ref = SectionRef.instance()
    name = "bucky"
    label, view = lit_views(vr, golden, name)[1]
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1, False)
    load(gpu, vox, tf, esl)
    assert p.esl == 1
    other = p.copy()
    other.esl, other.ray_threshold, other.light_kd = 0, 0.3, 0.0
    for j in range(3):
        other.view.light_pos[j] = 0.25 * (j + 1)
    for section_label, plane, clip in planes_of(view)[:3]:
        for mode in MODES:
            h = 0.0 if mode == "point" else half_width_of(p, name)
            want, _ = check(gpu, ref, (label, section_label, mode), vox, p, tf, plane, h, mode, None)
            out, depth = gpu.render_section(other, plane, h, mode, None, depth=True)
            assert diff(out, want) == 0 and depth_diff(depth, ref.render(p, vox, tf, plane, h, mode, None)[1]) == 0


@pytest.mark.parametrize("name", SECTION_VOLUMES)
def test_in_volume_equals_the_restatement(vr, gpu, golden, oracle, volumes, name):
    """vr_hip_render_section_in_volume_device equals render_section_device followed by render_backdrop_device in place on the GPU, and
    section_in_volume_render's frame and depth bits, with the depth buffer given and NULL; so do the host entry points.  Default mode
    (leaping, early termination) and full march of the composite pass."""
    import torch
    ref = SectionRef.instance()
    stream = torch.cuda.current_stream().cuda_stream
    loaded = False
    for v, (label, view) in enumerate(lit_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not loaded:
                load(gpu, vox, tf, esl)
                loaded = True
            shape = (p.out_rows, p.out_width)
            section_label, plane, _ = planes_of(view)[(v + sampling) % 5]
            mode = MODES[(v + sampling) % 4]
            h, window = (0.0 if mode == "point" else half_width_of(p, name)), (WINDOWS[name] if v % 2 else None)
            want, want_depth, want_section = ref.in_volume(p, vox, tf, esl, plane, h, mode, window)
            two = torch.full(shape + (4,), 77, dtype=torch.uint8, device="cuda")
            two_depth = torch.full(shape, 123.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                    # (the fills run on torch's stream, the frame on the context's)
            gpu.render_section_device(p, plane, h, mode, window, two.data_ptr(), two_depth.data_ptr(), stream)
            gpu.render_backdrop_device(p, two.data_ptr(), two_depth.data_ptr(), two.data_ptr(), stream)
            one = torch.full(shape + (4,), 78, dtype=torch.uint8, device="cuda")
            one_depth = torch.full(shape, 124.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                    # (the fills run on torch's stream, the frame on the context's)
            before = gpu.backdrop_frames(), gpu.section_frames()
            gpu.render_section_in_volume_device(p, plane, h, mode, window, one.data_ptr(), one_depth.data_ptr(), stream)
            own = torch.full(shape + (4,), 79, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                    # (the fill runs on torch's stream, the frame on the context's)
            gpu.render_section_in_volume_device(p, plane, h, mode, window, own.data_ptr(), None, stream)
            torch.cuda.synchronize()
            what = (name, label, sampling, full_march, section_label, mode)
            assert (gpu.backdrop_frames(), gpu.section_frames()) == (before[0] + 2, before[1] + 2), what
            assert torch.equal(one, two) and torch.equal(one_depth.view(torch.int32), two_depth.view(torch.int32)) and torch.equal(own, one), what
            assert diff(one.cpu().numpy(), want) == 0 and depth_diff(one_depth.cpu().numpy(), want_depth) == 0, (what, diff(one.cpu().numpy(), want))
            host, host_depth = gpu.render_section_in_volume(p, plane, h, mode, window, depth=True)
            assert diff(host, want) == 0 and depth_diff(host_depth, want_depth) == 0, what
            assert np.array_equal(gpu.render_section_in_volume(p, plane, h, mode, window), host), what


def test_in_volume_with_every_state(vr, gpu, golden, oracle, volumes):
    """Under clip `both`, the top light's grid at strength 0.6, PHONG and the pre-integration together: the section pass sees the clip and
    is unchanged by the other three; the composite pass sees all four"""
    name, clip = "bucky", CLIPS["both"]
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = SectionRef.instance(), ShadowRef.instance()
    q = None
    for v, (label, view) in enumerate(lit_views(vr, golden, name)):
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1, False)
        if q is None:
            load(gpu, vox, tf, esl)
            set_clip(gpu, clip)
            q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf, clip=clip)
        gpu.clear_shadow()
        gpu.clear_lighting()
        gpu.clear_preintegration()
        section_label, plane, _ = planes_of(view)[v % 5]
        mode = MODES[v % 4]
        h, window = (0.0 if mode == "point" else half_width_of(p, name)), (WINDOWS[name] if v % 2 else None)
        plain, plain_depth = gpu.render_section(p, plane, h, mode, window, depth=True)
        gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), 0.6)
        gpu.set_lighting(*PHONG)
        gpu.set_preintegration()
        out, depth = gpu.render_section_in_volume(p, plane, h, mode, window, depth=True)
        want, want_depth, want_section = ref.in_volume(p, vox, tf, esl, plane, h, mode, window, SLAB, clip, PHONG, q, 0.6)
        assert diff(out, want) == 0 and depth_diff(depth, want_depth) == 0, (label, section_label, mode, diff(out, want))
        alone, alone_depth = gpu.render_section(p, plane, h, mode, window, depth=True)
        assert diff(alone, want_section) == 0 and np.array_equal(alone, plain) and depth_diff(alone_depth, plain_depth) == 0, (label, mode)
    assert diff(want, want_section) > 0


def test_state_off_is_untouched(vr, gpu, golden, oracle, volumes):
    """A section is an argument, not state.  A plain default-mode frame (256 x 256: 128 tiles, under the measured-cost tile order), a MIP
    and an isosurface frame after section frames equal the frames before them; the composite still starts its tiles in the recorded order,
    the section frames start theirs in grid order; no other counter moves, section_frames counts"""
    ref, backdrop = SectionRef.instance(), BackdropRef.instance()
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    for k in range(3):
        first = gpu.render_volume(p)
    assert diff(first, backdrop.render(p, vox, tf, esl)) == 0 and gpu.last_launch()["ordered"] == 1
    fp = frame_params(vr, oracle, vox, p.view, 1, 1)
    mip, (iso, iso_depth) = gpu.render_mip(fp), gpu.render_iso(fp, 100.0, 4, depth=True)
    assert diff(mip, MipRef.instance().render(fp, vox, tf)[0]) == 0 and diff(iso, IsoRef.instance().render(fp, vox, tf, 100.0, 4)[0]) == 0
    counters = gpu.lighting_frames(), gpu.preint_frames(), gpu.shadow_builds()[0], gpu.backdrop_frames()
    count = gpu.section_frames()
    plane = planes_of(p.view)[1][1]
    for mode in MODES:
        h = 0.0 if mode == "point" else half_width_of(p, "bucky")
        check(gpu, ref, ("state off", mode), vox, p, tf, plane, h, mode, WINDOWS["bucky"])
        assert gpu.last_launch()["ordered"] == 0
    assert gpu.section_frames() == count + 8
    assert (gpu.lighting_frames(), gpu.preint_frames(), gpu.shadow_builds()[0], gpu.backdrop_frames()) == counters
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["ordered"] == 1
    again, (again_iso, again_depth) = gpu.render_mip(fp), gpu.render_iso(fp, 100.0, 4, depth=True)
    assert np.array_equal(again, mip) and np.array_equal(again_iso, iso) and depth_diff(again_depth, iso_depth) == 0
    assert gpu.section_frames() == count + 8
    out = gpu.render_section_in_volume(p, plane, 0.0, "point", WINDOWS["bucky"])
    assert diff(out, ref.in_volume(p, vox, tf, esl, plane, 0.0, "point", WINDOWS["bucky"])[0]) == 0
    assert gpu.section_frames() == count + 9 and gpu.backdrop_frames() == counters[3] + 1
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["ordered"] == 1


def test_errors(vr, gpu, golden, oracle, volumes):
    """Every error of step 10: a NULL section, a non-finite member, a normal of three zeros, mode > 3, half_width < 0, POINT with a half
    width, a thick mode without one, a window that is neither {0, 0} nor hi > lo, VR_SAMPLE_NEAREST — VR_ERR_INVALID from all four entry
    points, nothing counted; NULL buffers and params as for the isosurface"""
    import torch
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 3), 1, True)
    load(gpu, vox, tf, esl)
    L = vr.lib()
    buf = torch.zeros((80, 80, 4), dtype=torch.uint8, device="cuda")
    host = np.zeros((80, 80, 4), np.uint8)
    count = gpu.section_frames()
    nan, inf = float("nan"), float("inf")

    def section(plane=(0.0, 0.0, 1.0, 0.1), h=0.0, mode=0, window=(0.0, 0.0)):
        s = vr.VrSection()
        for i in range(4):
            s.plane[i] = plane[i]
        s.half_width, s.mode, s.window[0], s.window[1] = h, mode, window[0], window[1]
        return s

    def refused(params, sec):
        arg = None if sec is None else C.byref(sec)
        return [L.vr_hip_render_section_device(gpu._ctx, C.byref(params), arg, buf.data_ptr(), None, None),
                L.vr_hip_render_section(gpu._ctx, C.byref(params), arg, host.ctypes.data, None),
                L.vr_hip_render_section_in_volume_device(gpu._ctx, C.byref(params), arg, buf.data_ptr(), None, None),
                L.vr_hip_render_section_in_volume(gpu._ctx, C.byref(params), arg, host.ctypes.data, None)] == [1, 1, 1, 1]
    bad = [None, section(plane=(nan, 0.0, 1.0, 0.0)), section(plane=(0.0, inf, 1.0, 0.0)), section(plane=(0.0, 0.0, 1.0, nan)), section(h=nan, mode=1),
           section(h=inf, mode=1), section(window=(nan, 1.0)), section(window=(0.0, inf)), section(plane=(0.0, 0.0, 0.0, 0.5)), section(mode=4),
           section(h=-0.1, mode=1), section(h=0.1, mode=0), section(h=0.0, mode=1), section(h=0.0, mode=2), section(h=0.0, mode=3),
           section(window=(5.0, 5.0)), section(window=(9.0, 3.0)), section(window=(1.0, 0.0))]
    for i, sec in enumerate(bad):
        assert refused(p, sec), i
    nearest = p.copy()
    nearest.sampling = 0
    assert refused(nearest, section())
    with pytest.raises(vr.VrError) as e:
        gpu.render_section(nearest, (0.0, 0.0, 1.0, 0.0))
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    good = section(window=(0.0, 255.0))
    assert L.vr_hip_render_section_device(gpu._ctx, C.byref(p), C.byref(good), None, None, None) == 1
    assert L.vr_hip_render_section_device(gpu._ctx, None, C.byref(good), buf.data_ptr(), None, None) == 1
    assert L.vr_hip_render_section(gpu._ctx, C.byref(p), C.byref(good), None, None) == 1
    assert L.vr_hip_render_section_in_volume(gpu._ctx, C.byref(p), C.byref(good), None, None) == 1
    assert L.vr_hip_section_frames(gpu._ctx, None) == 1
    torch.cuda.synchronize()
    assert gpu.section_frames() == count
    assert L.vr_hip_render_section_device(gpu._ctx, C.byref(p), C.byref(good), buf.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert gpu.section_frames() == count + 1
    assert diff(buf.cpu().numpy(), SectionRef.instance().render(p, vox, tf, (0.0, 0.0, 1.0, 0.1), 0.0, "point", (0.0, 255.0))[0]) == 0


@needs_bounds_lib
def test_section_frames_under_the_bounds_checked_build():
    """A subset of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every gather address is
    held against its array — a violation fails the frame (VrError) — and the bytes still equal the restatement"""
    run_under_bounds_build(__file__, "edge_shapes or every_path or random_scenes or in_volume_with_every_state or (frames_equal and random_u16)", 7, timeout=900)


def test_driver_section_flags(golden, tmp_path):
    """volr_bench -section (HipRenderer::set_section through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance 2,
    256 x 256 — the restatement's frame for a POINT section under a window, and for the slab mean inside the volume with -shadow 17
    -preint, which the composite pass sees; what -section excludes is refused, and so are its options without it"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = SectionRef.instance()
    q = ShadowRef.instance().build(tuple(p.view.light_pos), 17, p.ray_step, vox, st["tf"])
    plane = (0.5, 0.5, 0.70703125, 0.125)              # (exact in fp32 and in the driver's decimal arguments)
    args = ["-section"] + [repr(c) for c in plane]
    alone = args + ["-section-window", "10", "250"]
    inside = args + ["-section-half", "0.125", "-section-mode", "mean", "-section-in-volume", "-shadow", "17", "-preint"]
    for extra in (alone, inside):
        out, rgb = run_driver(tmp_path, *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Section: plane" in out.stdout
        if extra is alone:
            want = ref.render(p, vox, st["tf"], plane, 0.0, "point", (10.0, 250.0))[0]
            assert (want[..., 3] == 255).sum() > 5000
        else:
            want, _, section = ref.in_volume(p, vox, st["tf"], st["esl"], plane, 0.125, "mean", None, SLAB, q=q, strength=1.0)
            assert diff(want, section) > 1000
        assert np.array_equal(rgb, want[..., :3]), (extra, int((rgb != want[..., :3]).any(axis=-1).sum()))
    for bad in (["-mip"], ["-iso", "100"], ["-hybrid", "100"], ["-devices", "0,0"], ["-r", "0"]):
        out, _ = run_driver(tmp_path, *bad, *args, size=(128, 128), pose=None, renderer=None if "-r" in bad else "1", output=None)
        assert out.returncode != 0 and "Error: -section" in out.stdout, (bad, out.stdout)
    for orphan in (["-section-window", "10", "250"], ["-section-half", "0.1"], ["-section-mode", "min"], ["-section-in-volume"]):
        out, _ = run_driver(tmp_path, *orphan, size=(128, 128), pose=None, output=None)
        assert out.returncode != 0 and "need -section" in out.stdout, (orphan, out.stdout)
