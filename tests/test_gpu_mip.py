"""GPU tier of the maximum-intensity projection (vr_hip_render_mip / vr_hip_render_mip_device): every frame the HIP path renders is
held byte for byte against mip_render of tests/feature_ref.c — the MIP loop restated with the CPU oracle's statics, which tests/test_mip_model.py
pins against the unmodified oracle.  Since esl on and esl off are both held against the same frame, they equal each other."""
import ctypes as C

import numpy as np
import pytest

from gpu_feature import MAPPINGS, diff, expected_bands, load, reset_context, run_driver
from mip_helpers import MipRef, ramp_tf, synthetic_volumes

pytestmark = pytest.mark.gpu

GOLDEN_VOLUMES = ("bucky", "blob_40x24x56", "shell48")
VOLUMES = GOLDEN_VOLUMES + ("random_u16", "late_max", "corner", "zeros", "first_slice")
SAMPLINGS = (0, 1, 2)                         # NEAREST, TRILINEAR, TRILINEAR_Q8
SIZES = ((80, 80), (120, 72))                 # 72 rows: not a multiple of the 16-row workgroup tile


@pytest.fixture(scope="module")
def volumes(golden):
    v = {name: np.ascontiguousarray(golden.voxels(name)) for name in GOLDEN_VOLUMES}
    v.update(synthetic_volumes())
    return v


@pytest.fixture(scope="module")
def tf():
    return ramp_tf()


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state or a forced path behind.  (Setting the layout drops the brick
    copies; every test that renders through the shared context begins with load or set_volume, which drops them anyway.)"""
    yield
    reset_context(vr, gpu)


def frame_params(vr, oracle, vox, view, sampling, esl):
    """Whole-frame parameters.  What a MIP frame must ignore is set to values that would show: threshold, light, and an ESL block
    geometry that is NOT the volume's (the kernel takes the grid of the min/max scan)."""
    z, y, x = vox.shape
    p = vr.VrParams()
    p.view = view
    p.ray_step = float(oracle.default_ray_step((x, y, z)))
    p.ray_threshold, p.light_kd = 0.5, 0.7
    p.esl, p.esl_block_dims = esl, 3
    for j in range(3):
        p.esl_block_size[j] = 0.1
    p.sampling = sampling
    return vr.whole_frame(p)


def views_of(vr, golden, index):
    """The eight benchmark views — at 80 x 80 and 120 x 72, alternating with `index` so that every volume sees both sizes and every
    view both across the volumes — and golden case 32's far perspective view, most of whose rays miss."""
    out = [(f"view{i}", vr.benchmark_view(*SIZES[(i + index) % 2], i)) for i in range(8)]
    far = golden.params(next(c for c in golden.cases() if c["id"] == 32)).view
    return out + [("far_persp", far)]


def expected(vr, oracle, vox, view, sampling, tf):
    return MipRef.instance().render(frame_params(vr, oracle, vox, view, sampling, 0), vox, tf)[0]


@pytest.mark.parametrize("name", VOLUMES)
def test_frames_equal_the_restatement_with_esl_off_and_on(vr, gpu, golden, oracle, volumes, tf, name):
    vox = volumes[name]
    load(gpu, vox, tf)
    hits = 0
    for label, view in views_of(vr, golden, VOLUMES.index(name)):
        for sampling in SAMPLINGS:
            ref = expected(vr, oracle, vox, view, sampling, tf)
            hits += int((ref[..., 3] != 0).sum())
            for esl in (0, 1):
                out = gpu.render_mip(frame_params(vr, oracle, vox, view, sampling, esl))
                assert diff(out, ref) == 0, (name, label, sampling, esl, diff(out, ref))
    assert hits > 10000            # the ramp transfer function makes every ray that hits the volume visible


def test_layouts_and_addressing_paths_agree(vr, gpu, golden, oracle, volumes, tf):
    """Linear array and brick copies (voxel, quad, oct), 32-bit tables, 64-bit tables and index arithmetic: the same frames"""
    seen = set()
    try:
        for name in ("blob_40x24x56", "random_u16"):
            vox = volumes[name]
            load(gpu, vox, tf)
            picked = [v for v in views_of(vr, golden, 0) if v[0] in ("view1", "view2", "view6", "far_persp")]
            for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
                gpu.set_layout(layout)
                planes = (-1, 5) if (layout == vr.LAYOUT_BRICKED and vox.dtype == np.uint16) else (-1,)      # 5: oct bricks for every view
                for plane in planes:
                    gpu.set_brick_plane(plane)
                    for wide in (0, 1, 2):
                        gpu.set_wide_addressing(wide)
                        for label, view in picked:
                            for sampling in SAMPLINGS:
                                ref = expected(vr, oracle, vox, view, sampling, tf)
                                for esl in (0, 1):
                                    out = gpu.render_mip(frame_params(vr, oracle, vox, view, sampling, esl))
                                    assert diff(out, ref) == 0, (name, layout, plane, wide, label, sampling, esl)
                                    seen.add(gpu.last_launch()["layout"])
    finally:
        gpu.set_wide_addressing(0)
        gpu.set_brick_plane(-1)
        gpu.set_layout(vr.LAYOUT_BRICKED)
    assert seen == {0, 1, 4, 5}, seen          # linear array, quad bricks, voxel bricks, oct bricks — and never a run or column copy


def test_tile_mappings_agree(vr, gpu, golden, oracle, volumes, tf):
    """Every lane order x wave shape, two phases of the tile grid: placement only"""
    vox = volumes["late_max"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(120, 72, 1)
    try:
        for sampling in (0, 1):
            ref = expected(vr, oracle, vox, view, sampling, tf)
            for lane_map, phase in MAPPINGS:
                gpu.set_tile_mapping(lane_map, *phase)
                out = gpu.render_mip(frame_params(vr, oracle, vox, view, sampling, 1))
                assert diff(out, ref) == 0, (sampling, lane_map % 4, lane_map // 4, phase)      # (lane order, wave shape)
                assert gpu.last_launch()["lane_map"] == lane_map
    finally:
        gpu.set_tile_mapping(-1)


def test_screen_partition(vr, gpu, golden, oracle, volumes, tf):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole frame"""
    vox = volumes["blob_40x24x56"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(80, 80, 5)
    for sampling in (0, 2):
        ref = expected(vr, oracle, vox, view, sampling, tf)
        p, per_rank = vr.band_partition(frame_params(vr, oracle, vox, view, sampling, 1), 1, 3, 16)
        assert (p.band_rows, p.band_stride, p.band_first) == (16, 3, 1)
        out = gpu.render_mip(p)
        assert out.shape[0] == per_rank * 16
        want = expected_bands(ref, 1, 3, 16, per_rank * 16)
        assert np.array_equal(out, want), (sampling, np.flatnonzero((out != want).any(axis=(1, 2))))      # (the local rows that differ)
        p = frame_params(vr, oracle, vox, view, sampling, 1)
        p.x0, p.out_width = 24, 40
        assert np.array_equal(gpu.render_mip(p), ref[:, 24:64]), sampling


def test_entry_points_and_error_conventions(vr, gpu, golden, oracle, volumes, tf):
    import torch
    vox = volumes["bucky"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(120, 72, 3)
    p = frame_params(vr, oracle, vox, view, 1, 1)
    ref = expected(vr, oracle, vox, view, 1, tf)
    host = gpu.render_mip(p)
    buf = torch.full((72, 120, 4), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                            # (the fill runs on torch's stream, the frame on the context's)
    gpu.timing_reset()
    for _ in range(3):
        gpu.render_mip_device(p, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 3                      # one launch per device-pointer frame, counted by vr_hip_timing
    assert np.array_equal(buf.cpu().numpy(), host) and diff(host, ref) == 0
    info = gpu.last_launch()
    assert info["tiles_x"] == 4 and info["tiles_y"] >= 5 and info["layout"] in (1, 5)
    L = vr.lib()
    assert L.vr_hip_render_mip(gpu._ctx, C.byref(p), None) == 1              # VR_ERR_INVALID, like vr_hip_render
    assert L.vr_hip_render_mip_device(gpu._ctx, C.byref(p), None, None) == 1
    assert L.vr_hip_render_mip(gpu._ctx, None, host.ctypes.data) == 1
    bad = p.copy()
    bad.sampling = 9
    with pytest.raises(vr.VrError) as e:
        gpu.render_mip(bad)
    assert e.value.code == 1
    fresh = vr.HipRenderer(0)
    try:
        fresh.set_window_buffer(128, 128)
        with pytest.raises(vr.VrError) as e:
            fresh.render_mip(p)
        assert e.value.code == 5                           # VR_ERR_NOT_READY: no volume
        fresh.set_volume(vox)
        with pytest.raises(vr.VrError) as e:
            fresh.render_mip(p)
        assert e.value.code == 5                           # ... no transfer function
        fresh.set_transfer_fn(tf, np.zeros(1024, np.uint32))
        assert diff(fresh.render_mip(p), ref) == 0
    finally:
        fresh.close()


def test_composited_frames_are_unchanged_around_mip_frames(vr, gpu, golden, oracle, volumes):
    case = next(c for c in golden.cases(True) if c["label"] == "bench64_view5_default")
    st = golden.volume_state("bucky")
    gpu.set_window_buffer(128, 128)
    gpu.set_transfer_fn(st["tf"], st["esl"])
    gpu.set_volume(golden.voxels("bucky"))
    for sampling in (0, 1):
        p = golden.params(case, sampling)
        before = gpu.render_volume(p)
        if sampling == 0:
            assert np.array_equal(before, golden.frame(case))
        for esl in (0, 1):
            q = p.copy()
            q.esl = esl
            mip = gpu.render_mip(q)
            assert diff(mip, MipRef.instance().render(golden.params(case, sampling), golden.voxels("bucky"), st["tf"])[0]) == 0
        assert np.array_equal(gpu.render_volume(p), before), sampling


def test_a_new_volume_brings_its_own_block_maxima(vr, gpu, golden, oracle, volumes, tf):
    """Volume A, then B on the same context: B's frames skip by B's maxima (A is bright where B is empty and the other way round)"""
    a, b = volumes["first_slice"], volumes["corner"]
    view = vr.benchmark_view(80, 80, 1)
    load(gpu, a, tf)
    for sampling in SAMPLINGS:
        assert diff(gpu.render_mip(frame_params(vr, oracle, a, view, sampling, 1)), expected(vr, oracle, a, view, sampling, tf)) == 0
    gpu.set_volume(b)
    fresh = vr.HipRenderer(0)
    try:
        load(fresh, b, tf)
        for sampling in SAMPLINGS:
            p = frame_params(vr, oracle, b, view, sampling, 1)
            out = gpu.render_mip(p)
            assert np.array_equal(out, fresh.render_mip(p)), sampling
            assert diff(out, expected(vr, oracle, b, view, sampling, tf)) == 0, sampling
    finally:
        fresh.close()


def test_release_linear_copy_keeps_skipping_frames_possible(vr, golden, oracle, volumes, tf):
    """The block maxima are scanned from the linear array: vr_hip_release_linear_copy derives them before it frees it"""
    vox = volumes["late_max"]
    view = vr.benchmark_view(80, 80, 6)
    r = vr.HipRenderer(0)
    try:
        load(r, vox, tf)
        for sampling in (0, 1):                            # esl off: builds the voxel and quad bricks, not the block maxima
            assert diff(r.render_mip(frame_params(vr, oracle, vox, view, sampling, 0)), expected(vr, oracle, vox, view, sampling, tf)) == 0
        r.release_linear_copy()
        assert r.volume_info().linear_resident == 0
        for sampling in (0, 1):
            assert diff(r.render_mip(frame_params(vr, oracle, vox, view, sampling, 1)), expected(vr, oracle, vox, view, sampling, tf)) == 0
    finally:
        r.close()


def test_driver_mip_flag(golden, tmp_path):
    """volr_bench -mip (HipRenderer::set_mip through the host mirror): Bucky.pvm, NEAREST, pose (-45,-45,0) at distance 2"""
    out, rgb = run_driver(tmp_path, "-mip", renderer="0")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Maximum-intensity projection" in out.stdout
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    ref = MipRef.instance().render(golden.params(case, 0), golden.voxels("bucky"), golden.volume_state("bucky")["tf"])[0]
    assert np.array_equal(rgb, ref[..., :3])
    assert not np.array_equal(ref, golden.frame(case))     # ... and it is not the composite
    out, _ = run_driver(tmp_path, "-mip", "-devices", "0,0", size=(128, 128), pose=None, renderer=None, output=None)
    assert out.returncode != 0 and "single device" in out.stdout
