"""GPU tier of the light-source shadows (vr_hip_set_shadow / vr_hip_multi_set_shadow): every light grid the HIP builder marches and every
shadowed composite frame is held byte for byte against shadow_build / shadow_render of tests/feature_ref.c, the contract of
include/vr_hip.h restated with the CPU oracle's statics.  tests/test_shadow_model.py ties that restatement to the pinned clipped composite and shows that the grids and frames compared
here are neither trivial nor unshadowed."""
import ctypes as C

import numpy as np
import pytest

from clip_helpers import BOTH, CLIPS, ClipRef, IDENTITY, composite_params, set_clip
from gpu_feature import PATH_VOLUMES, assert_order_repeats, diff, expected_bands, load, multi_pair, reset_context, run_driver, sweep_paths
from iso_helpers import all_volumes, frame_params, views_for
from shadow_helpers import COMPOSITE_VOLUMES, CUTOFF, FRAME_SCENES, GRID_SCENES, LIGHTS, SMALLEST, ShadowRef, unlit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return all_volumes(golden)


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


def fresh_grid(gpu, light, S, step, sampling=1, cutoff=CUTOFF):
    """the light grid built NOW by whatever path the context's knobs select: an identical set_shadow would keep the resident one"""
    before = gpu.shadow_builds()[0]
    gpu.clear_shadow()
    gpu.set_shadow(light, S, step, 1.0, cutoff, sampling)
    q = gpu.download_shadow()
    assert gpu.shadow_builds()[0] == before + 1
    return q


@pytest.mark.parametrize("name,light,S", GRID_SCENES + (SMALLEST,), ids=lambda v: str(v))
def test_light_grid_equals_the_restatement(vr, gpu, golden, oracle, volumes, name, light, S):
    """vr_hip_download_shadow against shadow_build: u8, u16 and the non-cubic blob, the three lights, S = 2 / 9 / 17 / 33, both builder
    samplings, VR_LAYOUT_LINEAR and bricked, every addressing path of vr_hip_set_wide_addressing"""
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, name)
    ref = ShadowRef.instance()
    load(gpu, vox, tf, esl)
    try:
        for sampling in (1, 2):
            want = ref.build(LIGHTS[light], S, p.ray_step, vox, tf, sampling=sampling)
            for layout, wide in ((vr.LAYOUT_BRICKED, 0), (vr.LAYOUT_BRICKED, 1), (vr.LAYOUT_BRICKED, 2), (vr.LAYOUT_BRICKED, 4), (vr.LAYOUT_LINEAR, 0), (vr.LAYOUT_LINEAR, 1)):
                if sampling == 2 and (layout, wide) not in ((vr.LAYOUT_BRICKED, 0), (vr.LAYOUT_LINEAR, 0)):
                    continue
                gpu.set_layout(layout)
                gpu.set_wide_addressing(wide)
                q = fresh_grid(gpu, LIGHTS[light], S, p.ray_step, sampling)
                assert q.shape == (S, S, S)
                bad = int((q != want).sum())
                assert bad == 0, (name, light, S, sampling, layout, wide, bad, int(np.abs(q.astype(int) - want.astype(int)).max()))
    finally:
        gpu.set_wide_addressing(0)
        gpu.set_layout(vr.LAYOUT_BRICKED)


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", COMPOSITE_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """Nine views x {default mode, full march} x {lit, light_kd = 0} x strength {1, 0.6}, all eight: the restatement's bytes; strength 0: the bytes of
    the same frame with the shadow cleared.  set_shadow(step=None): the wrapper resolves the step to the frame's ray_step."""
    light, S = FRAME_SCENES[name]
    ref = ShadowRef.instance()
    loaded, q = False, None
    for label, view in views_for(vr, golden, name):
        for full_march, lit, strength in ((f, l, s) for f in (False, True) for l in (True, False) for s in (1.0, 0.6)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if not lit:
                p = unlit(p)
            if not loaded:
                load(gpu, vox, tf, esl)
                q = ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
                loaded = True
            gpu.set_shadow(LIGHTS[light], S, None, strength)
            out = gpu.render_volume(p)
            info = gpu.last_launch()
            want = ref.render(p, vox, tf, esl, q, strength)
            assert diff(out, want) == 0, (name, sampling, label, full_march, lit, strength, diff(out, want), info)
            assert info["shadowed"] == 1 and info["layout"] in (0, 1, 5), info
        vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, True)
        gpu.set_shadow(LIGHTS[light], S, None, 0.0)
        zero = gpu.render_volume(p)
        assert gpu.last_launch()["shadowed"] == 1
        gpu.clear_shadow()
        assert np.array_equal(zero, gpu.render_volume(p)) and gpu.last_launch()["shadowed"] == 0, (name, sampling, label)
        assert diff(zero, ref.render(p, vox, tf, esl)) == 0


def test_the_smallest_grid_in_a_frame(vr, gpu, golden, oracle, volumes):
    """S = 2: every sample of the frame interpolates the one cell of the grid"""
    name, light, S = SMALLEST
    ref = ShadowRef.instance()
    for i, (label, view) in enumerate(views_for(vr, golden, name)):
        vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, 1, False)
        if i == 0:
            load(gpu, vox, tf, esl)
            gpu.set_shadow(LIGHTS[light], S, p.ray_step)
        q = ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
        want = ref.render(p, vox, tf, esl, q, 1.0)
        assert diff(gpu.render_volume(p), want) == 0, label
    assert np.array_equal(gpu.download_shadow().ravel(), q.ravel()) and ((q != 0) & (q != 255)).any()


def test_every_path_agrees_under_a_shadow(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / +4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, and never a run copy or a column window; u8 and u16 (oct bricks)"""
    ref = ShadowRef.instance()
    for name, expect in PATH_VOLUMES:
        light, S = FRAME_SCENES[name]
        views = [v for v in views_for(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for label, view in views:
            for sampling, full_march in ((1, True), (2, False)):
                vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
                q = ref.build(LIGHTS[light], S, p.ray_step, vox, tf)
                cases.append((label, sampling, p, ref.render(p, vox, tf, esl, q, 1.0)))
        load(gpu, vox, tf, esl)
        gpu.set_shadow(LIGHTS[light], S, p.ray_step)
        seen = set()

        def check(what):
            for label, sampling, p, want in cases:
                out = gpu.render_volume(p)
                info = gpu.last_launch()
                assert diff(out, want) == 0, (name, what, label, sampling, diff(out, want), info)
                assert info["layout"] in (0, 1, 5) and info["shadowed"] == 1, (name, what, label, sampling, info)
                seen.add(info["layout"])
        sweep_paths(vr, gpu, check)
        assert seen == expect, (name, seen)


def test_tile_order_repeats(vr, gpu, golden, oracle, volumes):
    """Default mode under the measured-cost tile order (256 x 256: 128 tiles): the same shadowed parameters four times give equal frames"""
    name = "bucky"
    light, S = FRAME_SCENES[name]
    ref = ShadowRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(256, 256, 1), 1, False)
    load(gpu, vox, tf, esl, (256, 256))
    gpu.set_shadow(LIGHTS[light], S, p.ray_step)
    want = ref.render(p, vox, tf, esl, ref.build(LIGHTS[light], S, p.ray_step, vox, tf), 1.0)
    assert_order_repeats(gpu, lambda: gpu.render_volume(p), want)


def test_screen_partition_and_entry_points(vr, gpu, golden, oracle, volumes):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole shadowed frame; the
    host-pointer entry point renders a frame of 1 MiB as two row slices that share ONE light grid; the device-pointer entry point runs on
    the caller's stream"""
    import torch
    name = "blob_40x24x56"
    light, S = FRAME_SCENES[name]
    ref = ShadowRef.instance()
    vox, whole, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), 1, True)
    load(gpu, vox, tf, esl)
    q = ref.build(LIGHTS[light], S, whole.ray_step, vox, tf)
    want = ref.render(whole, vox, tf, esl, q, 1.0)
    assert want.any()
    gpu.set_shadow(LIGHTS[light], S, whole.ray_step)
    p, per_rank = vr.band_partition(whole.copy(), 1, 3, 16)
    out = gpu.render_volume(p)
    assert out.shape[0] == per_rank * 16
    expected = expected_bands(want, 1, 3, 16, per_rank * 16)
    assert np.array_equal(out, expected), np.flatnonzero((out != expected).any(axis=(1, 2)))      # (the local rows that differ)
    crop = whole.copy()
    crop.x0, crop.out_width = 24, 40
    assert np.array_equal(gpu.render_volume(crop), want[:, 24:64])
    # the device-pointer entry point on the caller's stream: one launch
    buf = torch.full((72, 120, 4), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                            # (the fill runs on torch's stream, the frame on the context's)
    gpu.timing_reset()
    gpu.render_volume_device(whole, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and diff(buf.cpu().numpy(), want) == 0
    # 512 x 512 x 4 bytes = 1 MiB: two row slices on two streams of the context, the first of which builds the grid
    vox, big, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(512, 512, 1), 1, False)
    gpu.set_window_buffer(512, 512)
    gpu.clear_shadow()
    gpu.set_shadow(LIGHTS[light], S, big.ray_step)
    builds = gpu.shadow_builds()[0]
    gpu.timing_reset()
    out = gpu.render_volume(big)
    assert gpu.timing().launches == 2 and gpu.shadow_builds()[0] == builds + 1
    assert diff(out, ref.render(big, vox, tf, esl, q, 1.0)) == 0


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
def test_shadow_with_clip(vr, gpu, golden, oracle, volumes, clip_name):
    """Light rays are clipped like view rays: the grid downloaded after set_clip equals the restatement's clipped build, and differs from
    the unclipped one; the frames equal the restatement"""
    name, clip = "bucky", CLIPS[clip_name]
    light, S = FRAME_SCENES[name]
    ref = ShadowRef.instance()
    for i, (label, view) in enumerate(views_for(vr, golden, name)):
        for sampling, full_march in ((1, False), (2, True)):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
            if i == 0 and sampling == 1:
                load(gpu, vox, tf, esl)
                gpu.set_shadow(LIGHTS[light], S, p.ray_step)
                plain = gpu.download_shadow()
                set_clip(gpu, clip)
                q = gpu.download_shadow()
                want_q = ref.build(LIGHTS[light], S, p.ray_step, vox, tf, clip=clip)
                assert np.array_equal(q, want_q) and not np.array_equal(q, plain), clip_name
            out = gpu.render_volume(p)
            want = ref.render(p, vox, tf, esl, want_q, 1.0, clip)
            assert diff(out, want) == 0, (clip_name, label, sampling, full_march, diff(out, want))
    assert diff(want, ClipRef.instance().composite(p, vox, tf, esl, clip)) > 0


def test_staleness(vr, gpu, golden, oracle, volumes):
    """After set_transfer_fn, set_volume, set_clip and a changed set_shadow the next download differs from the one before and equals the
    restatement; an identical set_shadow, an identical set_clip and a second download build nothing (vr_hip_shadow_builds)"""
    ref = ShadowRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky")
    light, S, step = LIGHTS["top"], 17, float(p.ray_step)
    load(gpu, vox, tf, esl)
    gpu.clear_shadow()
    builds = gpu.shadow_builds()[0]
    gpu.set_shadow(light, S, step)
    assert gpu.shadow_builds()[0] == builds                       # lazily: nothing yet
    last = gpu.download_shadow()
    assert np.array_equal(last, ref.build(light, S, step, vox, tf)) and gpu.shadow_builds()[0] == builds + 1
    gpu.set_shadow(light, S, step)
    assert np.array_equal(gpu.download_shadow(), last) and gpu.shadow_builds()[0] == builds + 1
    gpu.set_shadow(light, S, step, 0.3)                            # the strength alone: the grid does not depend on it
    assert np.array_equal(gpu.download_shadow(), last) and gpu.shadow_builds()[0] == builds + 1
    gpu.set_shadow(light, S, step)
    tf2 = np.array(tf, np.float32).reshape(128, 4).copy()
    tf2 *= 0.5                                                    # half the alpha everywhere (premultiplied: the colours with it)
    other_vox = volumes["shell48"]
    steps = [("set_transfer_fn", lambda: gpu.set_transfer_fn(tf2, esl), lambda: ref.build(light, S, step, vox, tf2)),
             ("set_volume", lambda: gpu.set_volume(other_vox), lambda: ref.build(light, S, step, other_vox, tf2)),
             ("set_clip", lambda: set_clip(gpu, BOTH), lambda: ref.build(light, S, step, other_vox, tf2, clip=BOTH)),
             ("set_shadow", lambda: gpu.set_shadow(LIGHTS["outside"], S, step), lambda: ref.build(LIGHTS["outside"], S, step, other_vox, tf2, clip=BOTH))]
    for n, (what, change, expect) in enumerate(steps):
        change()
        q = gpu.download_shadow()
        assert not np.array_equal(q, last) and np.array_equal(q, expect()), what
        assert gpu.shadow_builds()[0] == builds + 2 + n, what
        last = q
    set_clip(gpu, BOTH)                                           # the same clip again: nothing is stale
    assert np.array_equal(gpu.download_shadow(), last) and gpu.shadow_builds()[0] == builds + 1 + len(steps)
    assert gpu.shadow_builds()[1] > 0.0


def test_state_off_returns_to_the_column_march(vr, gpu, golden, oracle, volumes):
    """An orthogonal full-march frame along z: the column march (layout 7) without a shadow, a quad / linear / oct copy with shadowed == 1
    under it, the column march and the first frame's bytes again after clear_shadow"""
    ref = ShadowRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(80, 80, 0), 1, True)
    load(gpu, vox, tf, esl)
    gpu.clear_shadow()
    first = gpu.render_volume(p)
    assert gpu.last_launch()["layout"] == 7 and gpu.last_launch()["shadowed"] == 0
    gpu.set_shadow(LIGHTS["top"], 17)                             # step=None: the next frame's ray_step, resolved once
    with pytest.raises(vr.VrError):
        gpu.download_shadow()                                     # no step yet
    builds = gpu.shadow_builds()[0]
    out = gpu.render_volume(p)
    info = gpu.last_launch()
    assert info["shadowed"] == 1 and info["layout"] in (0, 1, 5), info
    want_q = ref.build(LIGHTS["top"], 17, p.ray_step, vox, tf)
    assert diff(out, ref.render(p, vox, tf, esl, want_q, 1.0)) == 0
    finer = p.copy()
    finer.ray_step = float(p.ray_step) * 0.5                      # a later frame with another ray_step keeps the resolved step: no rebuild
    gpu.render_volume(finer)
    assert np.array_equal(gpu.download_shadow(), want_q) and gpu.shadow_builds()[0] == builds + 1
    gpu.clear_shadow()
    assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["layout"] == 7 and gpu.last_launch()["shadowed"] == 0


def test_errors_and_what_ignores_the_shadow(vr, gpu, golden, oracle, volumes):
    ref = ShadowRef.instance()
    vox, p, tf, esl = scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(120, 72, 3), 1, False)
    load(gpu, vox, tf, esl)
    L = vr.lib()
    good = vr.VrShadow((C.c_float * 3)(*LIGHTS["top"]), 17, float(p.ray_step), 1.0, CUTOFF, 1)
    assert L.vr_hip_set_shadow(None, C.byref(good)) == 1
    bad_values = [("light_pos", v) for v in (float("nan"), float("inf"))] + [("step", v) for v in (float("nan"), float("inf"), 0.0, -1.0, 1.0 / 8192.0)] + \
                 [("strength", v) for v in (float("nan"), -0.01, 1.01, float("inf"))] + [("cutoff", v) for v in (float("nan"), -0.01, 1.0, float("inf"))] + \
                 [("dims", v) for v in (0, 1, 257, 1 << 20)] + [("sampling", v) for v in (0, 3)]
    for member, value in bad_values:
        bad = vr.VrShadow.from_buffer_copy(good)
        if member == "light_pos":
            bad.light_pos[1] = value
        else:
            setattr(bad, member, value)
        assert L.vr_hip_set_shadow(gpu._ctx, C.byref(bad)) == 1, (member, value)                 # VR_ERR_INVALID
    for member, value in (("step", 1.0 / 4096.0), ("strength", 0.0), ("strength", 1.0), ("cutoff", 0.0), ("dims", 2), ("dims", 256), ("sampling", 2)):
        ok = vr.VrShadow.from_buffer_copy(good)
        setattr(ok, member, value)
        assert L.vr_hip_set_shadow(gpu._ctx, C.byref(ok)) == 0, (member, value)
    gpu.clear_shadow()
    with pytest.raises(vr.VrError) as e:
        gpu.set_shadow(LIGHTS["top"], dims=1)
    assert e.value.code == 1 and "dims" in str(e.value)
    plain = gpu.render_volume(p)                                  # a refused shadow changes nothing: still none
    assert diff(plain, ref.render(p, vox, tf, esl)) == 0 and gpu.last_launch()["shadowed"] == 0
    with pytest.raises(vr.VrError) as e:
        gpu.download_shadow()                                     # no shadow
    assert e.value.code == 5
    assert L.vr_hip_set_shadow(gpu._ctx, C.byref(good)) == 0
    small, dims = np.zeros(17 ** 3 - 1, np.uint8), C.c_uint32(0)
    assert L.vr_hip_download_shadow(gpu._ctx, small.ctypes.data, small.nbytes, C.byref(dims)) == 1 and dims.value == 17       # a short buffer
    empty = vr.HipRenderer(0)
    try:
        empty.set_shadow(LIGHTS["top"], 17, 0.01)
        with pytest.raises(vr.VrError) as e:
            empty.download_shadow()                               # no volume
        assert e.value.code == 5
        empty.set_volume(vox)
        with pytest.raises(vr.VrError) as e:
            empty.download_shadow()                               # no transfer function
        assert e.value.code == 5
    finally:
        empty.close()
    # NEAREST composite frames are refused, with the shadow still in place for the next TRILINEAR frame
    with pytest.raises(vr.VrError) as e:
        gpu.render_volume(scene(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(120, 72, 3), 0, False)[1])
    assert e.value.code == 1 and "shadow" in str(e.value)
    want = ref.render(p, vox, tf, esl, ref.build(LIGHTS["top"], 17, p.ray_step, vox, tf), 1.0)
    assert diff(gpu.render_volume(p), want) == 0 and diff(want, plain) > 0
    # MIP and isosurface frames ignore the state, NEAREST included
    for sampling in (0, 1):
        fp = frame_params(vr, oracle, vox, vr.benchmark_view(120, 72, 3), sampling, 1)
        with_shadow = [gpu.render_mip(fp)] + ([gpu.render_iso(fp, 100.0, 4)] if sampling else [])
        gpu.clear_shadow()
        without = [gpu.render_mip(fp)] + ([gpu.render_iso(fp, 100.0, 4)] if sampling else [])
        assert all(np.array_equal(a, b) and a.any() for a, b in zip(with_shadow, without)), sampling
        assert L.vr_hip_set_shadow(gpu._ctx, C.byref(good)) == 0


@pytest.mark.parametrize("transport", ("peer", "rccl-self"))
def test_multi_device_frames_are_shadowed(vr, gpu, golden, oracle, volumes, monkeypatch, transport):
    """MultiRenderer([0, 0]).set_shadow equals the single-context shadowed frame (and so the restatement), by peer copies and through RCCL
    with one communicator; every device's context builds its own grid"""
    name = "bucky"
    light, S = FRAME_SCENES[name]
    ref = ShadowRef.instance()
    with multi_pair(vr, monkeypatch, transport) as m:
        for sampling in (1, 2):
            vox, p, tf, esl = scene(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 72, 5), sampling, False)
            if sampling == 1:
                load(gpu, vox, tf, esl)
                m.set_transfer_fn(tf, esl)
                m.set_volume(vox)
            m.clear_shadow()
            gpu.clear_shadow()
            plain = gpu.render_volume(p)
            assert np.array_equal(m.render_volume(p), plain), sampling
            m.set_shadow(LIGHTS[light], S)
            gpu.set_shadow(LIGHTS[light], S)
            single = gpu.render_volume(p)
            assert diff(single, ref.render(p, vox, tf, esl, ref.build(LIGHTS[light], S, p.ray_step, vox, tf), 1.0)) == 0 and diff(single, plain) > 0
            assert np.array_equal(m.render_volume(p), single), sampling
        with pytest.raises(vr.VrError) as e:
            m.set_shadow(LIGHTS[light], 1)
        assert e.value.code == 1


def test_driver_shadow_flag(golden, tmp_path):
    """volr_bench -shadow 17 (HipRenderer::set_shadow through the host mirror, the light taken from the view): Bucky.pvm, TRILINEAR, pose
    (-45,-45,0) at distance 2, 256 x 256 — the frame the library call gives; and -shadow-strength"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    ref = ShadowRef.instance()
    q = ref.build(tuple(p.view.light_pos), 17, p.ray_step, vox, st["tf"])
    for extra, strength in (([], 1.0), (["-shadow-strength", "0.5"], 0.5)):
        out, rgb = run_driver(tmp_path, "-shadow", "17", *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Shadow: 17^3 nodes" in out.stdout
        want = ref.render(p, vox, st["tf"], st["esl"], q, strength)
        assert np.array_equal(rgb, want[..., :3]), (extra, int((rgb != want[..., :3]).any(axis=-1).sum()))
        assert diff(want, ref.render(p, vox, st["tf"], st["esl"])) > 1000
    out, _ = run_driver(tmp_path, "-shadow", "1", size=(128, 128), pose=None)
    assert out.returncode != 0 and "dims" in out.stdout
