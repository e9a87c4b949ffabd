"""GPU tier of the depth frames and of picking (vr_hip_render_depth*, vr_hip_pick): every frame the depth_kernel family renders is held bit
for bit — depth, value and alpha, no tolerance anywhere — against depth_render of tests/depth_ref.c, the contract of include/vr_hip.h
restated with the CPU oracle's statics.  tests/test_depth_model.py ties that restatement's alpha to the composite restatements and shows
that the frames compared here carry surfaces and rays without one and tell four wrong readings of the contract apart."""
import ctypes as C

import numpy as np
import pytest

import feature_random as fr
from backdrop_helpers import BackdropRef
from clip_helpers import CLIPS, set_clip
from depth_helpers import DEPTH_VOLUMES, MODES, OPACITIES, DepthRef, alpha_byte, check, classify, depth_launch, tier_frames
from gpu_feature import PATH_VOLUMES, depth_diff, diff, expected_bands, load, needs_bounds_lib, reset_context, run_driver, run_under_bounds_build, sweep_paths
from light_helpers import PHONG, lit_views, lit_volumes
from shadow_helpers import LIGHTS
from slab_helpers import POINT, SLAB, slab_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout or a forced path behind"""
    yield
    reset_context(vr, gpu)


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", DEPTH_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """The list of depth_helpers.tier_frames — nine views, two frames each: point and slab classification, the default mode and the full
    march, the ray step and four times it, no clip, box, plane and both — in the three modes at both opacities of the volume: depth, value
    and alpha bits, one frame counted each"""
    ref = DepthRef.instance()
    loaded = False
    frames = surfaces = 0
    start = gpu.depth_frames()
    for what, vox, p, tf, esl, clip, cmode in tier_frames(vr, golden, oracle, volumes, name, sampling):
        if not loaded:
            load(gpu, vox, tf, esl)
            loaded = True
        set_clip(gpu, clip)
        classify(gpu, cmode)
        for opacity in OPACITIES[name]:
            for mode in MODES:
                want = check(gpu, ref, what, vox, p, tf, esl, opacity, mode, cmode, clip)
                frames, surfaces = frames + 1, surfaces + int(want.surface.sum())
    print(f"{name} sampling {sampling}: {frames} frames, {surfaces} surface pixels compared")
    assert frames == 108 and surfaces > 108 * 300 and gpu.depth_frames() == start + frames, (frames, surfaces)


def test_alpha_is_the_composite_frames_alpha_byte_on_the_device(vr, gpu, golden, oracle, volumes):
    """Consequence 6 on the device alone: render_volume_device under clip `both`, PHONG, a light grid at strength 0.6 and pre-integration —
    and under each of them switched off in turn — has alpha bytes equal to map_float_int of the depth frame's alpha under the same clip and
    classification; the shadow and the lighting change no bit of the depth frame"""
    import torch
    name = "bucky"
    stream = torch.cuda.current_stream().cuda_stream
    loaded = False
    compared = 0
    for v, (label, view) in enumerate(lit_views(vr, golden, name)[::2]):
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + v % 2, v % 2 == 1)
        if not loaded:
            load(gpu, vox, tf, esl)
            loaded = True
        shape = (p.out_rows, p.out_width)
        for clip_on, lit, shadowed, preint in ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 0, 0)):
            reset_context(vr, gpu)
            if clip_on:
                set_clip(gpu, CLIPS["both"])
            if preint:
                gpu.set_preintegration()
            plain = gpu.render_depth(p, 0.5, "first", value=True, alpha=True)
            if lit:
                gpu.set_lighting(*PHONG)
            if shadowed:
                gpu.set_shadow(LIGHTS["top"], 17, float(p.ray_step), 0.6)
            frame = torch.full(shape + (4,), 77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                    # (the fill runs on torch's stream, the frame on the context's)
            gpu._resolve_shadow(p.ray_step)
            gpu.render_volume_device(p, frame.data_ptr(), stream)
            torch.cuda.synchronize()
            depth, value, alpha = gpu.render_depth(p, 0.5, "first", value=True, alpha=True)
            byte = alpha_byte(alpha)
            got = frame.cpu().numpy()[..., 3]
            assert np.array_equal(got, byte), (label, clip_on, lit, shadowed, preint, int((got != byte).sum()))
            assert all(depth_diff(a, b) == 0 for a, b in zip(plain, (depth, value, alpha))), (label, "shadow or lighting changed a depth frame")
            compared += int((byte != 0).sum())
    assert compared > 30 * 500, compared


def test_every_path_agrees(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / 4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bits, never a run copy or a column window, never a measured order; u8
    and u16 (oct bricks); a FIRST frame of the default mode under point classification and a MEAN frame of the full march under slabs"""
    ref = DepthRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in lit_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for k, (label, view) in enumerate(views):
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + k % 2, False)
            cases.append((label, p, OPACITIES[name][0], "first", POINT))
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + k % 2, True)
            cases.append((label, p, OPACITIES[name][1], "mean", SLAB))
        load(gpu, vox, tf, esl)
        seen = set()

        def check_all(what):
            for label, p, opacity, mode, cmode in cases:
                classify(gpu, cmode)
                check(gpu, ref, (name, what, label), vox, p, tf, esl, opacity, mode, cmode)
                seen.add(gpu.last_launch()["layout"])
        sweep_paths(vr, gpu, check_all)
        assert seen == expect, (name, seen)


def test_bands_crop_and_device_entry_point(vr, gpu, golden, oracle, volumes):
    """Three ranks of interleaved 16-row bands (a view of 70 rows: 5 bands, so two ranks hold a band beyond the view, where the three
    buffers are -1 / -1 / 0) and a crop in x equal the matching rows / columns of the whole frame; the device entry point renders the
    same in one launch"""
    import torch
    name = "blob_40x24x56"
    ref = DepthRef.instance()
    vox, whole, tf, esl = slab_scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 70, 5), 1, False)
    load(gpu, vox, tf, esl)
    for mode, opacity in (("first", OPACITIES[name][0]), ("mean", OPACITIES[name][1])):
        want = ref.render(whole, vox, tf, esl, opacity, mode)
        assert want.surface.sum() > 1000 and (~want.surface & want.rays).sum() > 500
        beyond_seen = 0
        for rank in range(3):
            p, per_rank = vr.band_partition(whole.copy(), rank, 3, 16)
            rows = per_rank * 16
            assert p.out_rows == rows == 32
            depth, value, alpha = gpu.render_depth(p, opacity, mode, value=True, alpha=True)
            for got, full, beyond in ((depth, want.depth, -1), (value, want.value, -1), (alpha, want.alpha, 0)):
                assert depth_diff(got, expected_bands(full, rank, 3, 16, rows, beyond=beyond)) == 0, (mode, rank)
            beyond_seen += int((~expected_bands(np.ones(70, bool), rank, 3, 16, rows)).sum())
        assert beyond_seen == 96 - 70
        crop = whole.copy()
        crop.x0, crop.out_width = 24, 40
        depth, value, alpha = gpu.render_depth(crop, opacity, mode, value=True, alpha=True)
        assert depth_diff(depth, want.depth[:, 24:64]) == 0 and depth_diff(value, want.value[:, 24:64]) == 0 and depth_diff(alpha, want.alpha[:, 24:64]) == 0
        bufs = [torch.full((70, 120), 123.0, dtype=torch.float32, device="cuda") for _ in range(3)]
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()                        # (the fills run on torch's stream, the frame on the context's)
        gpu.timing_reset()
        before = gpu.depth_frames()
        gpu.render_depth_device(whole, opacity, mode, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), stream)
        torch.cuda.synchronize()
        assert gpu.timing().launches == 1 and gpu.depth_frames() == before + 1 and depth_launch(gpu.last_launch())
        for got, full in zip(bufs, (want.depth, want.value, want.alpha)):
            assert depth_diff(got.cpu().numpy(), full) == 0, mode


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65) from views 0, 1 and 5 at 48 x 40 under both clips of its
    frames, with their esl and thresholds: the three modes, the classification alternating"""
    ref = DepthRef.instance()
    gpu.set_window_buffer(*fr.EDGE_SIZE)
    frames = 0
    for i, shape in enumerate(fr.EDGE_SHAPES):
        s = fr.edge_scene(oracle, vr, shape, dtype)
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        for j, f in enumerate(s.frames):
            set_clip(gpu, f.clip)
            cmode = SLAB if (i + j) % 2 else POINT
            classify(gpu, cmode)
            for m, mode in enumerate(MODES):
                check(gpu, ref, (shape, dtype, f.view, f.clip_name, mode), s.vox, f.p, s.tf, s.esl, (0.2, 0.6)[(i + m) % 2], mode, cmode, f.clip)
                frames += 1
    assert frames == len(fr.EDGE_SHAPES) * len(fr.EDGE_VIEWS) * len(fr.EDGE_CLIPS) * 3


def test_results_do_not_depend_on_the_buffers_asked_for(vr, gpu, golden, oracle, volumes):
    """Depth alone, depth and value, depth and alpha, all three: the same bits — with no alpha buffer a FIRST ray may stop at its surface,
    which changes nothing that is stored; through the host and the device entry points"""
    import torch
    ref = DepthRef.instance()
    name = "bucky"
    stream = torch.cuda.current_stream().cuda_stream
    for v, (label, view) in enumerate(lit_views(vr, golden, name)[1::3]):
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + v % 2, v % 2 == 0)
        load(gpu, vox, tf, esl)
        classify(gpu, SLAB if v % 2 else POINT)
        for mode in MODES:
            for opacity in OPACITIES[name]:
                want = check(gpu, ref, (label, mode), vox, p, tf, esl, opacity, mode, SLAB if v % 2 else POINT)
                alone = gpu.render_depth(p, opacity, mode)
                with_value = gpu.render_depth(p, opacity, mode, value=True)
                with_alpha = gpu.render_depth(p, opacity, mode, alpha=True)
                assert depth_diff(alone, want.depth) == 0, (label, mode, opacity)
                assert depth_diff(with_value[0], want.depth) == 0 and depth_diff(with_value[1], want.value) == 0, (label, mode, opacity)
                assert depth_diff(with_alpha[0], want.depth) == 0 and depth_diff(with_alpha[1], want.alpha) == 0, (label, mode, opacity)
                d = torch.full((p.out_rows, p.out_width), 123.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()                # (the fill runs on torch's stream, the frame on the context's)
                gpu.render_depth_device(p, opacity, mode, d.data_ptr(), None, None, stream)
                torch.cuda.synchronize()
                assert depth_diff(d.cpu().numpy(), want.depth) == 0, (label, mode, opacity)


def test_pick(vr, gpu, golden, oracle, volumes):
    """64 pixels — the four corners, misses of the cube and rays without a surface among them — equal what the whole frame stores there:
    hit, k, value, alpha; position and voxel bits equal the restatement's; one frame is counted per pixel; the partition fields are ignored.
    The error cases: n > 256, a pixel outside the window, NULL pointers with n > 0; n = 0 is fine."""
    ref = DepthRef.instance()
    name = "bucky"
    rng = np.random.default_rng(77)
    L = vr.lib()
    cube_misses = 0
    for v, (label, view) in enumerate(lit_views(vr, golden, name)[::4]):
        cmode = SLAB if v % 2 else POINT
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + v % 2, v % 2 == 1)
        load(gpu, vox, tf, esl)
        classify(gpu, cmode)
        w, h = p.view.width, p.view.height
        pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 60), rng.integers(0, h, 60))]
        for mode, opacity in zip(MODES, (OPACITIES[name][1], 0.5, OPACITIES[name][0])):
            want = ref.render(p, vox, tf, esl, opacity, mode, cmode)
            frame = gpu.render_depth(p, opacity, mode, value=True, alpha=True)
            before = gpu.depth_frames()
            cropped = p.copy()
            cropped.x0, cropped.out_width, cropped.band_rows, cropped.band_stride, cropped.band_first = 5, 7, 3, 2, 1
            got = gpu.pick(cropped, pixels, opacity, mode)
            assert gpu.depth_frames() == before + 64 and len(got) == 64
            hits = 0
            for (x, y), g in zip(pixels, got):
                stored = tuple(float(a[y, x]) for a in frame)
                what = (label, mode, x, y, g, stored)
                assert g["hit"] == (stored[0] >= 0.0) == bool(want.surface[y, x]), what
                one = np.array([g["k"], g["value"], g["alpha"]], np.float32), np.array(g["position"] + g["voxel"], np.float32)
                assert depth_diff(one[0], np.array(stored, np.float32)) == 0 and depth_diff(one[1], want.pick[y, x]) == 0, what
                if not g["hit"]:
                    assert (g["k"], g["value"]) == (-1.0, -1.0) and not any(g["position"]) and not any(g["voxel"]), what
                hits += g["hit"]
            assert 5 <= hits <= 59, (label, mode, hits)
            cube_misses += sum(not want.rays[y, x] for x, y in pixels)
    assert cube_misses > 30, cube_misses
    d = vr.VrDepth(0.5, 0)
    xy, out = (C.c_uint32 * 514)(), (vr.VrPick * 257)()
    before = gpu.depth_frames()
    assert L.vr_hip_pick(gpu._ctx, C.byref(p), C.byref(d), 0, None, None) == 0
    assert L.vr_hip_pick(gpu._ctx, C.byref(p), C.byref(d), 257, xy, out) == 1
    assert L.vr_hip_pick(gpu._ctx, C.byref(p), C.byref(d), 1, None, out) == 1 and L.vr_hip_pick(gpu._ctx, C.byref(p), C.byref(d), 1, xy, None) == 1
    assert L.vr_hip_pick(gpu._ctx, None, C.byref(d), 1, xy, out) == 1 and L.vr_hip_pick(gpu._ctx, C.byref(p), None, 1, xy, out) == 1
    for x, y in ((w, 0), (0, h), (0xffffffff, 0)):
        xy[0], xy[1] = x, y
        assert L.vr_hip_pick(gpu._ctx, C.byref(p), C.byref(d), 1, xy, out) == 1, (x, y)
    assert gpu.depth_frames() == before
    with pytest.raises(vr.VrError) as e:
        gpu.pick(p, [(w, 0)], 0.5)
    assert e.value.code == 1 and "outside" in str(e.value)
    assert gpu.pick(p, [], 0.5) == [] and len(gpu.pick(p, [(3, 4)] * 256, 0.5, "peak")) == 256


def test_errors_and_what_a_depth_frame_ignores(vr, gpu, golden, oracle, volumes):
    """Every error of step 10 — a NULL struct, a NULL depth buffer, mode > 2, a non-finite opacity, one outside [0, 1], FIRST with opacity 0,
    VR_SAMPLE_NEAREST — is VR_ERR_INVALID from both entry points and from the pick, nothing counted; PEAK and MEAN take opacity 0.  light_kd
    and light_pos, a shadow and a lighting change no bit.  depth_frames counts; the lighting, pre-integration, backdrop and section counters
    do not move, and the composite frame around the depth frames keeps its bytes and its recorded tile order."""
    import torch
    ref = DepthRef.instance()
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    for k in range(3):
        first = gpu.render_volume(p)
    assert gpu.last_launch()["ordered"] == 1
    L = vr.lib()
    shape = (p.out_rows, p.out_width)
    buf = torch.zeros(shape, dtype=torch.float32, device="cuda")
    host = np.zeros(shape, np.float32)
    xy, picked = (C.c_uint32 * 2)(100, 100), (vr.VrPick * 1)()
    count = gpu.depth_frames()
    nan, inf = float("nan"), float("inf")

    def refused(params, d):
        dev, hst = vr.VrDepthOut(buf.data_ptr(), None, None), vr.VrDepthOut(host.ctypes.data, None, None)
        arg = None if d is None else C.byref(d)
        return [L.vr_hip_render_depth_device(gpu._ctx, C.byref(params), arg, C.byref(dev), None),
                L.vr_hip_render_depth(gpu._ctx, C.byref(params), arg, C.byref(hst)),
                L.vr_hip_pick(gpu._ctx, C.byref(params), arg, 1, xy, picked)]
    bad = [None, vr.VrDepth(0.5, 3), vr.VrDepth(nan, 0), vr.VrDepth(inf, 1), vr.VrDepth(-inf, 2), vr.VrDepth(-0.1, 1), vr.VrDepth(1.5, 0), vr.VrDepth(0.0, 0),
           vr.VrDepth(nan, 2)]
    for i, d in enumerate(bad):
        assert refused(p, d) == [1, 1, 1], i
    nearest = p.copy()
    nearest.sampling = 0
    assert refused(nearest, vr.VrDepth(0.5, 0)) == [1, 1, 1]
    with pytest.raises(vr.VrError) as e:
        gpu.render_depth(nearest, 0.5)
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    good = vr.VrDepth(0.5, 0)
    no_depth = vr.VrDepthOut(None, buf.data_ptr(), None)
    assert L.vr_hip_render_depth_device(gpu._ctx, C.byref(p), C.byref(good), C.byref(no_depth), None) == 1 and L.vr_hip_render_depth(gpu._ctx, C.byref(p), C.byref(good), C.byref(no_depth)) == 1
    assert L.vr_hip_render_depth_device(gpu._ctx, C.byref(p), C.byref(good), None, None) == 1 and L.vr_hip_render_depth(gpu._ctx, C.byref(p), C.byref(good), None) == 1
    assert L.vr_hip_render_depth_device(gpu._ctx, None, C.byref(good), C.byref(vr.VrDepthOut(buf.data_ptr(), None, None)), None) == 1
    assert L.vr_hip_depth_frames(gpu._ctx, None) == 1
    torch.cuda.synchronize()
    assert gpu.depth_frames() == count
    counters = gpu.lighting_frames(), gpu.preint_frames(), gpu.backdrop_frames(), gpu.section_frames()
    for mode in ("peak", "mean"):
        check(gpu, ref, ("opacity 0", mode), vox, p, tf, esl, 0.0, mode)
    want = check(gpu, ref, ("plain",), vox, p, tf, esl, 0.5, "first")
    assert gpu.depth_frames() == count + 3
    other = p.copy()
    other.light_kd = 0.0
    for j in range(3):
        other.view.light_pos[j] = 0.25 * (j + 1)
    gpu.set_lighting(*PHONG)
    gpu.set_shadow(LIGHTS["top"], 17, float(p.ray_step), 0.6)
    depth, value, alpha = gpu.render_depth(other, 0.5, "first", value=True, alpha=True)
    assert depth_diff(depth, want.depth) == 0 and depth_diff(value, want.value) == 0 and depth_diff(alpha, want.alpha) == 0
    gpu.clear_shadow()
    gpu.clear_lighting()
    assert gpu.depth_frames() == count + 4 and (gpu.lighting_frames(), gpu.preint_frames(), gpu.backdrop_frames(), gpu.section_frames()) == counters
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["ordered"] == 1


def test_the_first_depth_is_a_backdrop_layer(vr, gpu, golden, oracle, volumes):
    """The FIRST depth buffer with an opaque colour layer, fed to render_backdrop: the frame backdrop_render gives with that depth —
    the composite stops at the surface the depth frame found, and pixels without one (depth -1) are plain composite pixels"""
    ref, backdrop = DepthRef.instance(), BackdropRef.instance()
    name = "bucky"
    for v, (label, view) in enumerate(lit_views(vr, golden, name)[::3]):
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1 + v % 2, v % 2 == 1)
        load(gpu, vox, tf, esl)
        opacity = OPACITIES[name][v % 2]
        want = check(gpu, ref, (label, "layer"), vox, p, tf, esl, opacity, "first")
        depth = gpu.render_depth(p, opacity, "first")
        layer = np.empty((p.out_rows, p.out_width, 4), np.uint8)
        layer[...] = (40, 90, 200, 255)
        out = gpu.render_backdrop(p, layer, depth)
        expected = backdrop.render(p, vox, tf, esl, layer, np.array(want.depth))
        assert diff(out, expected) == 0, (label, diff(out, expected))
        assert diff(out, backdrop.render(p, vox, tf, esl)) > 300 and want.surface.sum() > 300, label


@needs_bounds_lib
def test_depth_frames_under_the_bounds_checked_build():
    """A subset of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every gather address is
    held against its array — a violation fails the frame (VrError) — and the bits still equal the restatement"""
    run_under_bounds_build(__file__, "edge_shapes or every_path or pick or (frames_equal and random_u16)", 6, timeout=900)


def test_driver_depth_flags(golden, tmp_path):
    """volr_bench -depth (HipRenderer::render_depth through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance 2,
    256 x 256 — the grey image is the restatement's FIRST depth of the hits, normalised over their range; -pick prints the restatement's
    pick of that pixel; NEAREST and a device list are refused, and -depth-mode and -pick need -depth"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = DepthRef.instance()
    for mode in ("first", "mean"):
        want = ref.render(p, vox, st["tf"], st["esl"], 0.5, mode)
        out, rgb = run_driver(tmp_path, "-depth", "0.5", "-depth-mode", mode, "-pick", "128", "128")
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Depth:" in out.stdout and want.surface.sum() > 5000
        d = want.depth[want.surface]
        lo, hi = np.float32(d.min()), np.float32(d.max())
        grey = np.zeros(want.depth.shape, np.uint8)
        scaled = ((want.depth[want.surface] - lo) / (hi - lo)).astype(np.float32)
        grey[want.surface] = (np.float32(255.0) - scaled * np.float32(254.0) + np.float32(0.5)).astype(np.uint8)
        assert np.array_equal(rgb[..., 0], grey) and np.array_equal(rgb[..., 1], grey) and np.array_equal(rgb[..., 2], grey), int((rgb[..., 0] != grey).sum())
        line = next(ln for ln in out.stdout.splitlines() if ln.startswith("Pick (128, 128):"))
        assert want.surface[128, 128] and f"k {float(want.depth[128, 128]):.9g}" in line and f"value {float(want.value[128, 128]):.9g}" in line, line
        assert "voxel (" + ", ".join(f"{float(c):.9g}" for c in want.pick[128, 128, 3:]) + ")" in line, line
    for bad in (["-devices", "0,0"], ["-r", "0"], ["-mip"]):
        out, _ = run_driver(tmp_path, *bad, "-depth", "0.5", size=(128, 128), pose=None, renderer=None if "-r" in bad else "1", output=None)
        assert out.returncode != 0 and "Error: -depth" in out.stdout, (bad, out.stdout)
    for orphan in (["-depth-mode", "peak"], ["-pick", "3", "4"]):
        out, _ = run_driver(tmp_path, *orphan, size=(128, 128), pose=None, output=None)
        assert out.returncode != 0 and "need -depth" in out.stdout, (orphan, out.stdout)
