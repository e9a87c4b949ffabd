"""GPU tier of the gradient lighting (vr_hip_set_lighting / vr_hip_multi_set_lighting): every lit composite frame the composite_lit kernels
render is held byte for byte against light_render of tests/feature_ref.c, the contract of include/vr_hip.h restated with the CPU oracle's statics.
tests/test_light_model.py ties that restatement to the pinned clipped composite and shows that the frames compared here are neither
trivial nor the cue-lit ones, and that the plateau volume takes the zero-gradient branch."""
import ctypes as C

import numpy as np
import pytest

from clip_helpers import CLIPS, ClipRef, IDENTITY, composite_params, set_clip
from gpu_feature import (PATH_VOLUMES, assert_order_repeats, diff, expected_bands, load, multi_pair, needs_bounds_lib, reset_context, run_driver,
                         run_under_bounds_build, sweep_paths)
from iso_helpers import frame_params
from light_helpers import IDENTITY_LIGHTING, LIGHTINGS, LIT_VOLUMES, PHONG, LightRef, cue, lit_views, lit_volumes
from shadow_helpers import FRAME_SCENES, LIGHTS, ShadowRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state or a forced path behind.  (Setting the layout drops the brick
    copies; every test that renders through the shared context begins with load or set_volume, which drops them anyway.)"""
    yield
    reset_context(vr, gpu)


def scene(vr, golden, oracle, volumes, name, view=None, sampling=1, full_march=False):
    """(voxels, params, tf, esl) of a volume's composite frame"""
    vox = volumes[name]
    p, tf, esl = composite_params(vr, golden, oracle, name, vox, view or vr.benchmark_view(80, 80, 0), sampling, full_march)
    return vox, p, tf, esl


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", LIT_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """Nine views x {default mode, full march} x the four LIGHTINGS: the restatement's bytes, on the gradient-lit kernels (layout 0, 1 or 5,
    one more lit frame counted each).  { 1, 0, 0, 4 }: the bytes of the GPU's own frame with light_kd = 0 and the lighting cleared.
    light_kd is ignored: a lit frame with light_kd = 0 has the same bytes."""
    ref = LightRef.instance()
    loaded = False
    for label, view in lit_views(vr, golden, name):
        for full_march in (False, True):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not loaded:
                load(gpu, vox, tf, esl)
                loaded = True
            for lighting in LIGHTINGS:
                gpu.set_lighting(*lighting)
                before = gpu.lighting_frames()
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                want = ref.render(p, vox, tf, esl, lighting)
                assert diff(out, want) == 0, (name, sampling, label, full_march, lighting, diff(out, want), info)
                assert info["layout"] in (0, 1, 5) and info["shadowed"] == 0 and gpu.lighting_frames() == before + 1, info
            assert np.array_equal(gpu.render_volume(cue(p)), out), (name, sampling, label, full_march, "light_kd")
            gpu.set_lighting(*IDENTITY_LIGHTING)
            same = gpu.render_volume(p)
            gpu.clear_lighting()
            before = gpu.lighting_frames()
            assert np.array_equal(same, gpu.render_volume(cue(p))) and gpu.lighting_frames() == before, (name, sampling, label, full_march, "identity")


def test_every_path_agrees_under_a_lighting(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9 (3, 4, 6, 7, 8 fall back), wide addressing 0 / 1 / 2 / +4,
    every lane order x wave shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, and never a run copy or a column
    window; u8 and u16 (oct bricks)"""
    ref = LightRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in lit_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for label, view in views:
            for sampling, full_march in ((1, True), (2, False)):
                vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
                cases.append((label, sampling, p, ref.render(p, vox, tf, esl, PHONG)))
        load(gpu, vox, tf, esl)
        gpu.set_lighting(*PHONG)
        seen = set()

        def check(what):
            for label, sampling, p, want in cases:
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                assert diff(out, want) == 0, (name, what, label, sampling, diff(out, want), info)
                assert info["layout"] in (0, 1, 5), (name, what, label, sampling, info)
                seen.add(info["layout"])
        sweep_paths(vr, gpu, check)
        assert seen == expect, (name, seen)


def test_tile_order_repeats(vr, gpu, golden, oracle, volumes):
    """Default mode under the measured-cost tile order (256 x 256: 128 tiles): the same lit parameters four times give equal frames"""
    ref = LightRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    gpu.set_lighting(*PHONG)
    want = ref.render(p, vox, tf, esl, PHONG)
    assert_order_repeats(gpu, lambda: gpu.render_volume(p), want)


def test_screen_partition_and_entry_points(vr, gpu, golden, oracle, volumes):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole lit frame; the
    device-pointer entry point runs on the caller's stream in one launch"""
    import torch
    name = "blob_40x24x56"
    ref = LightRef.instance()
    vox, whole, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), 1, True)
    load(gpu, vox, tf, esl)
    want = ref.render(whole, vox, tf, esl, PHONG)
    assert want.any()
    gpu.set_lighting(*PHONG)
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
    before = gpu.lighting_frames()
    gpu.render_volume_device(whole, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and diff(buf.cpu().numpy(), want) == 0 and gpu.lighting_frames() == before + 1


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
def test_lighting_with_clip(vr, gpu, golden, oracle, volumes, clip_name):
    """The lit kernels run clip_segment: under each of CLIPS the frames equal the restatement, and differ from the clipped cue-lit frame"""
    name, clip = "bucky", CLIPS[clip_name]
    ref = LightRef.instance()
    for i, (label, view) in enumerate(lit_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if i == 0 and sampling == 1:
                load(gpu, vox, tf, esl)
                gpu.set_lighting(*PHONG)
                set_clip(gpu, clip)
            out = gpu.render_volume(p)
            want = ref.render(p, vox, tf, esl, PHONG, clip=clip)
            assert diff(out, want) == 0, (clip_name, label, sampling, full_march, diff(out, want))
    assert diff(want, ClipRef.instance().composite(p, vox, tf, esl, clip)) > 0


@pytest.mark.parametrize("name", sorted(FRAME_SCENES))
def test_lighting_with_shadow(vr, gpu, golden, oracle, volumes, name):
    """The shadow's factor scales the colour after step 4: with the light grids of the shadow tests at strength 1 and 0 the frames equal the
    restatement (shadowed == 1, still on the lit kernels); strength 0 gives the bytes of the lit frame without a shadow"""
    light, S = FRAME_SCENES[name]
    ref, shadow_ref = LightRef.instance(), ShadowRef.instance()
    q = None
    for i, (label, view) in enumerate(lit_views(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if q is None:
                load(gpu, vox, tf, esl)
                gpu.set_lighting(*PHONG)
                q = shadow_ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
            for strength in (1.0, 0.0):
                gpu.set_shadow(LIGHTS[light], S, float(p.ray_step), strength)
                before = gpu.lighting_frames()
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                want = ref.render(p, vox, tf, esl, PHONG, q, strength)
                assert diff(out, want) == 0, (name, label, sampling, full_march, strength, diff(out, want), info)
                assert info["shadowed"] == 1 and info["layout"] in (0, 1, 5) and gpu.lighting_frames() == before + 1, info
            assert diff(want, ref.render(p, vox, tf, esl, PHONG)) == 0            # strength 0
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, lit_views(vr, golden, name)[1][1], 1, False)
    assert diff(ref.render(p, vox, tf, esl, PHONG, q, 1.0), ref.render(p, vox, tf, esl, PHONG)) > 0


def test_counter_and_state_off_returns_to_the_column_march(vr, gpu, golden, oracle, volumes):
    """An orthogonal full-march frame along z: the column march (layout 7) without a lighting; a quad / linear / oct copy and one counted
    frame under it; the column march, the first frame's bytes and an unchanged counter again after clear_lighting.  An identical
    set_lighting changes nothing; MIP and isosurface frames are not counted."""
    ref = LightRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 0), 1, True)
    load(gpu, vox, tf, esl)
    gpu.clear_lighting()
    count = gpu.lighting_frames()
    first = gpu.render_volume(p)
    assert gpu.last_launch()["layout"] == 7 and gpu.lighting_frames() == count
    gpu.set_lighting(*PHONG)
    assert gpu.lighting_frames() == count                         # setting it renders nothing
    out = gpu.render_volume(p)
    info = gpu.last_launch()
    assert info["layout"] in (0, 1, 5) and gpu.lighting_frames() == count + 1, info
    assert diff(out, ref.render(p, vox, tf, esl, PHONG)) == 0 and diff(out, first) > 0
    gpu.set_lighting(*PHONG)
    assert np.array_equal(gpu.render_volume(p), out) and gpu.lighting_frames() == count + 2
    fp = frame_params(vr, oracle, vox, vr.benchmark_view(80, 80, 0), 1, 1)
    gpu.render_mip(fp)
    gpu.render_iso(fp, 100.0, 4)
    assert gpu.lighting_frames() == count + 2
    gpu.clear_lighting()
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["layout"] == 7 and gpu.lighting_frames() == count + 2


def test_errors_and_what_ignores_the_lighting(vr, gpu, golden, oracle, volumes):
    ref = LightRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(120, 72, 3), 1, False)
    load(gpu, vox, tf, esl)
    L = vr.lib()
    good = vr.VrLighting(*[float(v) for v in PHONG[:3]], PHONG[3])
    assert L.vr_hip_set_lighting(None, C.byref(good)) == 1
    count = C.c_uint64(0)
    assert L.vr_hip_lighting_frames(None, C.byref(count)) == 1 and L.vr_hip_lighting_frames(gpu._ctx, None) == 1
    bad_values = [(m, v) for m in ("ambient", "diffuse", "specular") for v in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01)] + \
                 [("shininess_log2", v) for v in (11, 1 << 20, 0xffffffff)]
    for member, value in bad_values:
        bad = vr.VrLighting.from_buffer_copy(good)
        setattr(bad, member, value)
        assert L.vr_hip_set_lighting(gpu._ctx, C.byref(bad)) == 1, (member, value)                 # VR_ERR_INVALID
    for member, value in [(m, v) for m in ("ambient", "diffuse", "specular") for v in (0.0, 1.0)] + [("shininess_log2", 0), ("shininess_log2", 10)]:
        ok = vr.VrLighting.from_buffer_copy(good)
        setattr(ok, member, value)
        assert L.vr_hip_set_lighting(gpu._ctx, C.byref(ok)) == 0, (member, value)
    gpu.clear_lighting()
    with pytest.raises(vr.VrError) as e:
        gpu.set_lighting(0.2, 0.5, 0.5, 11)
    assert e.value.code == 1 and "shininess_log2" in str(e.value)
    plain = gpu.render_volume(p)                                  # a refused lighting changes nothing: still none
    assert diff(plain, ClipRef.instance().composite(p, vox, tf, esl, IDENTITY)) == 0
    assert L.vr_hip_set_lighting(gpu._ctx, C.byref(good)) == 0
    # NEAREST composite frames are refused, with the lighting still in place for the next TRILINEAR frame
    with pytest.raises(vr.VrError) as e:
        gpu.render_volume(scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(120, 72, 3), 0, False)[1])
    assert e.value.code == 1 and "lighting" in str(e.value)
    want = ref.render(p, vox, tf, esl, PHONG)
    assert diff(gpu.render_volume(p), want) == 0 and diff(want, plain) > 0
    # MIP and isosurface frames ignore the state, NEAREST included
    for sampling in (0, 1):
        fp = frame_params(vr, oracle, vox, vr.benchmark_view(120, 72, 3), sampling, 1)
        with_lighting = [gpu.render_mip(fp)] + ([gpu.render_iso(fp, 100.0, 4)] if sampling else [])
        gpu.clear_lighting()
        without = [gpu.render_mip(fp)] + ([gpu.render_iso(fp, 100.0, 4)] if sampling else [])
        assert all(np.array_equal(a, b) and a.any() for a, b in zip(with_lighting, without)), sampling
        assert L.vr_hip_set_lighting(gpu._ctx, C.byref(good)) == 0


@needs_bounds_lib
def test_lit_frames_under_the_bounds_checked_build():
    """The frames, paths, clip and shadow tests of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py):
    every gather address of the six gradient fetches is held against its array — a violation fails the frame (VrError) — and the bytes
    still equal the restatement"""
    run_under_bounds_build(__file__, "frames_equal_the_restatement or every_path or with_clip or with_shadow", 15, timeout=600)


@pytest.mark.parametrize("transport", ("peer", "rccl-self"))
def test_multi_device_frames_are_lit(vr, gpu, golden, oracle, volumes, monkeypatch, transport):
    """MultiRenderer([0, 0]).set_lighting equals the single-context lit frame (and so the restatement), by peer copies and through RCCL
    with one communicator"""
    name = "bucky"
    ref = LightRef.instance()
    with multi_pair(vr, monkeypatch, transport) as m:
        for sampling in (1, 2):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), sampling, False)
            if sampling == 1:
                load(gpu, vox, tf, esl)
                m.set_transfer_fn(tf, esl)
                m.set_volume(vox)
            m.clear_lighting()
            gpu.clear_lighting()
            plain = gpu.render_volume(p)
            assert np.array_equal(m.render_volume(p), plain), sampling
            m.set_lighting(*PHONG)
            gpu.set_lighting(*PHONG)
            single = gpu.render_volume(p)
            assert diff(single, ref.render(p, vox, tf, esl, PHONG)) == 0 and diff(single, plain) > 0
            assert np.array_equal(m.render_volume(p), single), sampling
        with pytest.raises(vr.VrError) as e:
            m.set_lighting(0.5, 1.5, 0.0, 0)
        assert e.value.code == 1


def test_driver_phong_flag(golden, tmp_path):
    """volr_bench -phong ka kd ks n (HipRenderer::set_lighting through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance
    2, 256 x 256 — the frame the library call gives; with -shadow 17 the two compose; a refused lighting ends the driver"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = LightRef.instance()
    q = ShadowRef.instance().build(tuple(p.view.light_pos), 17, p.ray_step, vox, st["tf"])
    for extra, grid in (([], None), (["-shadow", "17"], q)):
        out, rgb = run_driver(tmp_path, "-phong", "0.25", "0.65", "0.4", "4", *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Lighting: ambient 0.25, diffuse 0.65, specular 0.4, shininess 2^4" in out.stdout
        want = ref.render(p, vox, st["tf"], st["esl"], PHONG, grid, 1.0)
        assert np.array_equal(rgb, want[..., :3]), (extra, int((rgb != want[..., :3]).any(axis=-1).sum()))
        assert diff(want, ClipRef.instance().composite(p, vox, st["tf"], st["esl"], IDENTITY)) > 1000
    out, _ = run_driver(tmp_path, "-phong", "0.25", "0.65", "0.4", "11", size=(128, 128), pose=None)
    assert out.returncode != 0 and "shininess_log2" in out.stdout
