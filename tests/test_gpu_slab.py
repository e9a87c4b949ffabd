"""GPU tier of the pre-integrated classification (vr_hip_set_preintegration / vr_hip_multi_set_preintegration): every slab-classified
composite frame the composite_slab and composite_slab_lit kernels render is held byte for byte against slab_render of tests/feature_ref.c, the contract of
include/vr_hip.h restated with the CPU oracle's statics.  tests/test_slab_model.py ties that restatement to the pinned clipped, shadowed
and gradient-lit composites and shows that the frames compared here take both branches and are not the point-classified ones."""
import ctypes as C

import numpy as np
import pytest

from clip_helpers import CLIPS, ClipRef, IDENTITY, set_clip
from feature_random import EDGE_DTYPES, EDGE_SHAPES, edge_scene
from gpu_feature import (PATH_VOLUMES, assert_order_repeats, diff, expected_bands, load, multi_pair, needs_bounds_lib, reset_context, run_driver,
                         run_under_bounds_build, sweep_paths)
from iso_helpers import IsoRef, frame_params
from light_helpers import IDENTITY_LIGHTING, LIGHTINGS, PHONG, cue
from mip_helpers import MipRef, ramp_tf
from shadow_helpers import FRAME_SCENES, LIGHTS, ShadowRef
from slab_helpers import DENSE_CUT, POINT, SLAB, SLAB_VOLUMES, SlabRef, holed_tf, phase_scene, slab_scene, slab_views, slab_volumes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return slab_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state or a forced path behind.  (Setting the layout drops the brick
    copies; every test that renders through the shared context begins with load or set_volume, which drops them anyway.)"""
    yield
    reset_context(vr, gpu)


def scene(vr, golden, oracle, volumes, name, view=None, sampling=1, full_march=False, step_factor=1):
    return slab_scene(vr, golden, oracle, volumes, name, view or vr.benchmark_view(80, 80, 0), sampling, full_march, step_factor)


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", SLAB_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """Nine views x {default mode, full march} x {the ray step, four times it: the clamping variant} x {cue-lit, light_kd = 0}: the
    restatement's bytes, on the slab kernels (layout 0, 1 or 5, one more slab frame counted each).  On the plateau whole waves skip the
    empty samples in front of the block and the first block sample needs the coordinate of a skipped one; on the ramp a peak of the
    transfer function lies between consecutive samples."""
    ref = SlabRef.instance()
    loaded = False
    frames = shown = 0
    for label, view in slab_views(vr, golden, name):
        for full_march in (False, True):
            for factor in (1, 4):
                vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march, factor)
                if not loaded:
                    load(gpu, vox, tf, esl)
                    gpu.set_preintegration()
                    loaded = True
                for params in (p, cue(p)):
                    before = gpu.preint_frames()
                    out = gpu.render_volume(params)
                    info = gpu.last_launch()
                    want = ref.render(params, vox, tf, esl, SLAB)
                    assert diff(out, want) == 0, (name, sampling, label, full_march, factor, params.light_kd, diff(out, want), info)
                    assert info["layout"] in (0, 1, 5) and info["shadowed"] == 0 and gpu.preint_frames() == before + 1, info
                    frames, shown = frames + 1, shown + int(want.any(axis=-1).sum())
    print(f"{name} sampling {sampling}: {frames} frames, {shown} non-empty pixels compared")
    assert frames == 72 and shown > 72 * 500, (frames, shown)


@pytest.mark.parametrize("sampling", (1, 2))
def test_phase_scene(vr, gpu, sampling):
    """The phase-independence scene of tests/test_slab_model.py, slab and point classified: the restatement's bytes both ways"""
    ref = SlabRef.instance()
    vox, p, tf, esl, window = phase_scene(vr, sampling)
    load(gpu, vox, tf, esl)
    gpu.set_preintegration()
    slab = gpu.render_volume(p)
    gpu.clear_preintegration()
    point = gpu.render_volume(p)
    assert diff(slab, ref.render(p, vox, tf, esl, SLAB)) == 0 and diff(point, ref.render(p, vox, tf, esl, POINT)) == 0
    assert diff(slab[window], point[window]) > 100


@pytest.mark.parametrize("dtype", EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65) from views 0, 1 and 5 under both clips of its frames:
    the cue-lit slab frame, and the slab frame under the lighting and the light grid of those frames"""
    ref, shadow_ref = SlabRef.instance(), ShadowRef.instance()
    gpu.set_window_buffer(64, 64)
    for shape in EDGE_SHAPES:
        s = edge_scene(oracle, vr, shape, dtype)
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        gpu.set_preintegration()
        for f in s.frames:
            set_clip(gpu, f.clip)
            gpu.clear_lighting()
            gpu.clear_shadow()
            out = gpu.render_volume(f.p)
            want = ref.render(f.p, s.vox, s.tf, s.esl, SLAB, f.clip)
            assert diff(out, want) == 0, (shape, dtype, f.view, f.clip_name, "cue", diff(out, want), gpu.last_launch())
            q = shadow_ref.build(f.light, f.S, f.shadow_step, s.vox, s.tf, sampling=f.shadow_sampling, clip=f.clip)
            gpu.set_lighting(*f.lighting)
            gpu.set_shadow(f.light, f.S, float(f.shadow_step), f.strength, sampling=f.shadow_sampling)
            out = gpu.render_volume(f.p)
            want = ref.render(f.p, s.vox, s.tf, s.esl, SLAB, f.clip, f.lighting, q, f.strength)
            assert diff(out, want) == 0, (shape, dtype, f.view, f.clip_name, "lit and shadowed", diff(out, want), gpu.last_launch())


def test_every_path_agrees_under_preintegration(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9 (3, 4, 6, 7, 8 fall back), wide addressing 0 / 1 / 2 / +4,
    every lane order x wave shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, and never a run copy or a column
    window; u8 and u16 (oct bricks); the cue-lit family and, under a lighting, the lit one"""
    ref = SlabRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in slab_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for label, view in views:
            for sampling, full_march in ((1, True), (2, False)):
                vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
                cases.append((label, sampling, p, ref.render(p, vox, tf, esl, SLAB), ref.render(p, vox, tf, esl, SLAB, lighting=PHONG)))
        load(gpu, vox, tf, esl)
        gpu.set_preintegration()
        seen = set()

        def check(what):
            for label, sampling, p, want, want_lit in cases:
                for lighting, expected in ((None, want), (PHONG, want_lit)):
                    if lighting is None:
                        gpu.clear_lighting()
                    else:
                        gpu.set_lighting(*lighting)
                    out = gpu.render_volume(p)
                    info = gpu.last_launch()
                    assert diff(out, expected) == 0, (name, what, label, sampling, lighting, diff(out, expected), info)
                    assert info["layout"] in (0, 1, 5), (name, what, label, sampling, info)
                    seen.add(info["layout"])
        sweep_paths(vr, gpu, check)
        assert seen == expect, (name, seen)


def test_tile_order_repeats(vr, gpu, golden, oracle, volumes):
    """Default mode under the measured-cost tile order (256 x 256: 128 tiles): the same slab parameters four times give equal frames"""
    ref = SlabRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    gpu.set_preintegration()
    want = ref.render(p, vox, tf, esl, SLAB)
    assert_order_repeats(gpu, lambda: gpu.render_volume(p), want)


def test_screen_partition_and_entry_points(vr, gpu, golden, oracle, volumes):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole slab frame; the
    device-pointer entry point runs on the caller's stream in one launch"""
    import torch
    name = "blob_40x24x56"
    ref = SlabRef.instance()
    vox, whole, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), 1, True)
    load(gpu, vox, tf, esl)
    want = ref.render(whole, vox, tf, esl, SLAB)
    assert want.any()
    gpu.set_preintegration()
    p, per_rank = vr.band_partition(whole.copy(), 1, 3, 16)
    out = gpu.render_volume(p)
    assert out.shape[0] == per_rank * 16
    expected = expected_bands(want, 1, 3, 16, per_rank * 16)
    assert np.array_equal(out, expected), np.flatnonzero((out != expected).any(axis=(1, 2)))      # (the local rows that differ)
    crop = whole.copy()
    crop.x0, crop.out_width = 24, 40
    assert np.array_equal(gpu.render_volume(crop), want[:, 24:64])
    buf = torch.full((72, 120, 4), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                            # (the fill runs on torch's stream, the frame on the context's)
    gpu.timing_reset()
    before = gpu.preint_frames()
    gpu.render_volume_device(whole, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and diff(buf.cpu().numpy(), want) == 0 and gpu.preint_frames() == before + 1


ALL_CLIPS = dict(CLIPS, dense_cut=DENSE_CUT)


@pytest.mark.parametrize("clip_name", sorted(ALL_CLIPS))
def test_preintegration_with_clip(vr, gpu, golden, oracle, volumes, clip_name):
    """The slab kernels run clip_segment: under each of CLIPS, and under a plane whose cut face lies in dense matter — a first sample inside
    a gradient, whose slab is empty by the tp = tb rule —, the frames equal the restatement and differ from the clipped point-classified frame"""
    name, clip = "bucky", ALL_CLIPS[clip_name]
    ref = SlabRef.instance()
    for i, (label, view) in enumerate(slab_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if i == 0 and sampling == 1:
                load(gpu, vox, tf, esl)
                gpu.set_preintegration()
                set_clip(gpu, clip)
            out = gpu.render_volume(p)
            want = ref.render(p, vox, tf, esl, SLAB, clip)
            assert diff(out, want) == 0, (clip_name, label, sampling, full_march, diff(out, want))
    assert diff(want, ClipRef.instance().composite(p, vox, tf, esl, clip)) > 0


@pytest.mark.parametrize("name", sorted(FRAME_SCENES))
def test_preintegration_with_shadow(vr, gpu, golden, oracle, volumes, name):
    """The shadow's factor scales the slab's colour: with the light grids of the shadow tests at strength 1, 0.6 and 0 the frames equal the
    restatement (shadowed == 1, on the slab kernels); strength 0 gives the bytes of the slab frame without a shadow.  The grid itself is
    point classified: it is the shadow tests' grid, and toggling the pre-integration does not rebuild it."""
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = SlabRef.instance(), ShadowRef.instance()
    q = None
    for i, (label, view) in enumerate(slab_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if q is None:
                load(gpu, vox, tf, esl)
                gpu.set_preintegration()
                q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
            for strength in (1.0, 0.6, 0.0):
                gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), strength)
                before = gpu.preint_frames()
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                want = ref.render(p, vox, tf, esl, SLAB, q=q, strength=strength)
                assert diff(out, want) == 0, (name, label, sampling, full_march, strength, diff(out, want), info)
                assert info["shadowed"] == 1 and info["layout"] in (0, 1, 5) and gpu.preint_frames() == before + 1, info
            assert diff(want, ref.render(p, vox, tf, esl, SLAB)) == 0            # strength 0
    builds = gpu.shadow_builds()[0]
    gpu.clear_preintegration()
    gpu.render_volume(p)
    gpu.set_preintegration()
    gpu.render_volume(p)
    assert gpu.shadow_builds()[0] == builds
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, slab_views(vr, golden, name)[1][1], 1, False)
    assert diff(ref.render(p, vox, tf, esl, SLAB, q=q, strength=1.0), ref.render(p, vox, tf, esl, SLAB)) > 0


@pytest.mark.parametrize("name", ("bucky", "plateau", "random_u16"))
def test_preintegration_with_lighting(vr, gpu, golden, oracle, volumes, name):
    """The gradient lighting sees the slab's colour (composite_slab_lit): each of LIGHTINGS gives the restatement's bytes, lit frames and
    slab frames both counted; { 1, 0, 0, 4 } gives the bytes of the GPU's own slab frame with light_kd = 0"""
    ref = SlabRef.instance()
    loaded = False
    for label, view in slab_views(vr, golden, name):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not loaded:
                load(gpu, vox, tf, esl)
                gpu.set_preintegration()
                loaded = True
            for lighting in LIGHTINGS:
                gpu.set_lighting(*lighting)
                before = gpu.preint_frames(), gpu.lighting_frames()
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                want = ref.render(p, vox, tf, esl, SLAB, lighting=lighting)
                assert diff(out, want) == 0, (name, label, sampling, full_march, lighting, diff(out, want), info)
                assert info["layout"] in (0, 1, 5) and (gpu.preint_frames(), gpu.lighting_frames()) == (before[0] + 1, before[1] + 1), info
            gpu.set_lighting(*IDENTITY_LIGHTING)
            same = gpu.render_volume(p)
            gpu.clear_lighting()
            assert np.array_equal(same, gpu.render_volume(cue(p))), (name, label, sampling, full_march, "identity")


def test_clip_shadow_and_lighting_together(vr, gpu, golden, oracle, volumes):
    """All four states at once, both families' worth: under the clip `both` with the top light's grid (built under that clip: light rays are
    clipped too) at strength 0.6, cue-lit and under { 0.25, 0.65, 0.4, 4 }"""
    name, clip = "bucky", CLIPS["both"]
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = SlabRef.instance(), ShadowRef.instance()
    q = None
    for label, view in slab_views(vr, golden, name):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if q is None:
                load(gpu, vox, tf, esl)
                gpu.set_preintegration()
                set_clip(gpu, clip)
                q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf, clip=clip)
                gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), 0.6)
            for lighting in (None, PHONG):
                if lighting is None:
                    gpu.clear_lighting()
                else:
                    gpu.set_lighting(*lighting)
                out = gpu.render_volume(p)
                want = ref.render(p, vox, tf, esl, SLAB, clip, lighting, q, 0.6)
                assert diff(out, want) == 0, (label, sampling, full_march, lighting, diff(out, want), gpu.last_launch())
    assert want.any()


def test_state_counter_and_what_ignores_it(vr, gpu, golden, oracle, volumes):
    """On, off, on again: an orthogonal full-march frame along z takes the column march (layout 7) and the oracle's bytes without the state,
    a quad / linear / oct copy and one counted frame under it, and the column march, the first frame's bytes and an unchanged counter again
    after clear_preintegration.  An identical set changes nothing; on = 2 is VR_ERR_INVALID and leaves the state; NEAREST composite frames
    are refused with the state still in place; MIP and isosurface frames ignore it (their restatements' bytes) and are not counted."""
    ref = SlabRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 0), 1, True)
    load(gpu, vox, tf, esl)
    gpu.clear_preintegration()
    count = gpu.preint_frames()
    first = gpu.render_volume(p)
    assert gpu.last_launch()["layout"] == 7 and gpu.preint_frames() == count
    assert diff(first, oracle.render(p, vox, tf, esl)) == 0
    gpu.set_preintegration()
    assert gpu.preint_frames() == count                           # setting it renders nothing
    out = gpu.render_volume(p)
    info = gpu.last_launch()
    assert info["layout"] in (0, 1, 5) and gpu.preint_frames() == count + 1, info
    assert diff(out, ref.render(p, vox, tf, esl, SLAB)) == 0 and diff(out, first) > 0
    gpu.set_preintegration(True)
    assert np.array_equal(gpu.render_volume(p), out) and gpu.preint_frames() == count + 2
    L = vr.lib()
    with pytest.raises(vr.VrError) as e:
        gpu.set_preintegration(2)
    assert e.value.code == 1 and "pre-integration" in str(e.value)
    assert L.vr_hip_set_preintegration(gpu._ctx, 0xffffffff) == 1 and L.vr_hip_preint_frames(gpu._ctx, None) == 1
    assert np.array_equal(gpu.render_volume(p), out) and gpu.preint_frames() == count + 3      # a refused value changes nothing: still on
    with pytest.raises(vr.VrError) as e:
        gpu.render_volume(scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 0), 0, True)[1])
    assert e.value.code == 1 and "pre-integration" in str(e.value) and gpu.preint_frames() == count + 3
    for sampling in (0, 1):
        fp = frame_params(vr, oracle, vox, vr.benchmark_view(80, 80, 3), sampling, 1)
        assert diff(gpu.render_mip(fp), MipRef.instance().render(fp, vox, tf)[0]) == 0
        if sampling:
            assert diff(gpu.render_iso(fp, 100.0, 4), IsoRef.instance().render(fp, vox, tf, 100.0, 4)[0]) == 0
    assert gpu.preint_frames() == count + 3
    gpu.clear_preintegration()
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["layout"] == 7 and gpu.preint_frames() == count + 3
    gpu.set_preintegration()
    assert np.array_equal(gpu.render_volume(p), out) and gpu.preint_frames() == count + 4


def test_integral_table_as_uploaded(vr, gpu, golden):
    """download_tf_integral equals the restatement's K bit for bit for the default (Bucky's), the ramp and the holed transfer function"""
    ref = SlabRef.instance()
    esl = golden.volume_state("bucky")["esl"]
    for tf in (golden.volume_state("bucky")["tf"], ramp_tf(), holed_tf()):
        gpu.set_transfer_fn(tf, esl)
        got, want = gpu.download_tf_integral(), ref.integral(tf)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and want.any()
    fresh = vr.HipRenderer(0)
    try:
        with pytest.raises(vr.VrError) as e:
            fresh.download_tf_integral()
        assert e.value.code == 5                                  # VR_ERR_NOT_READY
    finally:
        fresh.close()


def test_holed_transfer_function(vr, gpu, golden, oracle, volumes):
    """Slabs that end inside a hole of the transfer function (tb in the hole, tp not: NOT transparent), on a transfer function with and
    without leading zeros: random_u16 and the blob under the holed and the ramp transfer function"""
    ref = SlabRef.instance()
    for name in ("random_u16", "blob_40x24x56"):
        for tf in (holed_tf(), ramp_tf()):
            loaded = False
            for label, view in slab_views(vr, golden, name)[:4]:
                vox, p, _, esl = scene(vr, golden, oracle, volumes, name, view, 1, True)
                p.ray_threshold = 0.95
                if not loaded:
                    load(gpu, vox, tf, esl)
                    gpu.set_preintegration()
                    loaded = True
                out = gpu.render_volume(p)
                want = ref.render(p, vox, tf, esl, SLAB)
                assert diff(out, want) == 0 and want.any(), (name, label, diff(out, want), gpu.last_launch())


@needs_bounds_lib
def test_slab_frames_under_the_bounds_checked_build():
    """The frame, path and state tests of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py):
    every gather address is held against its array — a violation fails the frame (VrError) — and the bytes still equal the restatement"""
    run_under_bounds_build(__file__, "frames_equal_the_restatement or edge_shapes or every_path or with_clip or with_shadow or with_lighting or together or state_counter",
                           25, timeout=900)


@pytest.mark.parametrize("transport", ("peer", "rccl-self"))
def test_multi_device_frames_are_slab_classified(vr, gpu, golden, oracle, volumes, monkeypatch, transport):
    """MultiRenderer([0, 0]).set_preintegration equals the single-context slab frame (and so the restatement), by peer copies and through
    RCCL with one communicator"""
    name = "bucky"
    ref = SlabRef.instance()
    with multi_pair(vr, monkeypatch, transport) as m:
        for sampling in (1, 2):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), sampling, False)
            if sampling == 1:
                load(gpu, vox, tf, esl)
                m.set_transfer_fn(tf, esl)
                m.set_volume(vox)
            m.set_preintegration(False)
            gpu.clear_preintegration()
            plain = gpu.render_volume(p)
            assert np.array_equal(m.render_volume(p), plain), sampling
            m.set_preintegration()
            gpu.set_preintegration()
            single = gpu.render_volume(p)
            assert diff(single, ref.render(p, vox, tf, esl, SLAB)) == 0 and diff(single, plain) > 0
            assert np.array_equal(m.render_volume(p), single), sampling
        with pytest.raises(vr.VrError) as e:
            m.set_preintegration(2)
        assert e.value.code == 1


def test_driver_preint_flag(golden, tmp_path):
    """volr_bench -preint (HipRenderer::set_preintegration through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance 2,
    256 x 256 — the frame the library call gives; with -shadow 17 -phong 0.25 0.65 0.4 4 the three compose"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = SlabRef.instance()
    q = ShadowRef.instance().build(tuple(p.view.light_pos), 17, p.ray_step, vox, st["tf"])
    for extra, lighting, grid in (([], None, None), (["-shadow", "17", "-phong", "0.25", "0.65", "0.4", "4"], PHONG, q)):
        out, rgb = run_driver(tmp_path, "-preint", *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Classification: pre-integrated (slab)" in out.stdout
        want = ref.render(p, vox, st["tf"], st["esl"], SLAB, lighting=lighting, q=grid, strength=1.0)
        assert np.array_equal(rgb, want[..., :3]), (extra, int((rgb != want[..., :3]).any(axis=-1).sum()))
        assert diff(want, ref.render(p, vox, st["tf"], st["esl"], POINT, lighting=lighting, q=grid, strength=1.0)) > 1000
