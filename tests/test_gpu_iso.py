"""GPU tier of the shaded isosurface with depth (vr_hip_render_iso / vr_hip_render_iso_device): every frame and every depth buffer the
HIP path renders is held byte for byte / bit for bit against iso_render of tests/feature_ref.c — the contract restated with the CPU oracle's statics,
which tests/test_iso_model.py holds against the MIP restatement and an analytic sphere.  Since esl on and esl off are both held against
the same frame, they equal each other."""
import ctypes as C

import numpy as np
import pytest

from gpu_feature import MAPPINGS, depth_diff, diff, expected_bands, load, reset_context, run_driver
from iso_helpers import NO_SURFACE, PAIRS, IsoRef, all_volumes, depth_bits, frame_params, views_for
from mip_helpers import MipRef, ramp_tf

pytestmark = pytest.mark.gpu

SAMPLINGS = (1, 2)                            # TRILINEAR, TRILINEAR_Q8
REFINE = 4


@pytest.fixture(scope="module")
def volumes(golden):
    return all_volumes(golden)


@pytest.fixture(scope="module")
def tf():
    return ramp_tf()


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state or a forced path behind.  (Setting the layout drops the brick
    copies; every test that renders through the shared context begins with load or set_volume, which drops them anyway.)"""
    yield
    reset_context(vr, gpu)


def expected(vr, oracle, vox, view, sampling, tf, level, light_kd=0.7, refine=REFINE):
    return IsoRef.instance().render(frame_params(vr, oracle, vox, view, sampling, 0, light_kd), vox, tf, level, refine)


def check(gpu, p, level, ref, what, refine=REFINE):
    """one frame with depth against (frame, depth) of the restatement"""
    out, depth = gpu.render_iso(p, level, refine, depth=True)
    assert diff(out, ref[0]) == 0 and depth_diff(depth, ref[1]) == 0, (what, diff(out, ref[0]), depth_diff(depth, ref[1]))
    return out, depth


@pytest.mark.parametrize("name,level", PAIRS, ids=[f"{n}@{int(l)}" for n, l in PAIRS])
def test_frames_and_depths_equal_the_restatement_with_esl_off_and_on(vr, gpu, golden, oracle, volumes, tf, name, level):
    vox = volumes[name]
    load(gpu, vox, tf)
    hits = 0
    for label, view in views_for(vr, golden, name):
        for sampling in SAMPLINGS:
            ref = expected(vr, oracle, vox, view, sampling, tf, level)
            hits += ref[2]["hits"]
            for esl in (0, 1):
                check(gpu, frame_params(vr, oracle, vox, view, sampling, esl), level, ref, (name, level, label, sampling, esl))
    # one unlit pass per volume: no gradient is fetched, the pixel is the base colour
    label, view = views_for(vr, golden, name)[1]
    ref = expected(vr, oracle, vox, view, 1, tf, level, light_kd=0.0)
    for esl in (0, 1):
        check(gpu, frame_params(vr, oracle, vox, view, 1, esl, light_kd=0.0), level, ref, (name, level, label, "unlit", esl))
    assert (hits == 0) == ((name, level) in NO_SURFACE), hits          # the test cannot pass on empty frames


def test_the_pairs_hold_enough_surface(vr, golden, oracle, volumes, tf):
    """... nor on nearly empty ones: the surface pixels of the expected frames above (the restatement keeps them: nothing is rendered twice)"""
    hits = {(name, level): sum(expected(vr, oracle, volumes[name], view, sampling, tf, level)[2]["hits"]
                               for _, view in views_for(vr, golden, name) for sampling in SAMPLINGS) for name, level in PAIRS}
    assert sum(hits.values()) > 300000, hits


def test_layouts_and_addressing_paths_agree(vr, gpu, golden, oracle, volumes, tf):
    """Linear array and brick copies (quad, oct), 32-bit tables, 64-bit tables and index arithmetic: the same frames and depths"""
    seen = set()
    try:
        for name, level in (("blob_40x24x56", 100.0), ("random_u16", 200.0 * 257)):
            vox = volumes[name]
            load(gpu, vox, tf)
            picked = [v for v in views_for(vr, golden, name) if v[0] in ("view1", "view2", "view6", "far_persp")]
            for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
                gpu.set_layout(layout)
                planes = (-1, 5) if (layout == vr.LAYOUT_BRICKED and vox.dtype == np.uint16) else (-1,)      # 5: oct bricks for every view
                for plane in planes:
                    gpu.set_brick_plane(plane)
                    for wide in (0, 1, 2):
                        gpu.set_wide_addressing(wide)
                        for label, view in picked:
                            for sampling in SAMPLINGS:
                                ref = expected(vr, oracle, vox, view, sampling, tf, level)
                                for esl in (0, 1):
                                    check(gpu, frame_params(vr, oracle, vox, view, sampling, esl), level, ref, (name, layout, plane, wide, label, sampling, esl))
                                    seen.add(gpu.last_launch()["layout"])
    finally:
        gpu.set_wide_addressing(0)
        gpu.set_brick_plane(-1)
        gpu.set_layout(vr.LAYOUT_BRICKED)
    assert seen == {0, 1, 5}, seen          # linear array, quad bricks, oct bricks — and never a run, voxel or column copy


def test_tile_mappings_agree(vr, gpu, golden, oracle, volumes, tf):
    """Every lane order x wave shape, two phases of the tile grid: placement only"""
    vox = volumes["late_max"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(120, 72, 1)
    try:
        ref = expected(vr, oracle, vox, view, 1, tf, 24.5)
        assert ref[2]["hits"] > 1000
        for lane_map, phase in MAPPINGS:
            gpu.set_tile_mapping(lane_map, *phase)
            check(gpu, frame_params(vr, oracle, vox, view, 1, 1), 24.5, ref, (lane_map % 4, lane_map // 4, phase))      # (lane order, wave shape)
            assert gpu.last_launch()["lane_map"] == lane_map
    finally:
        gpu.set_tile_mapping(-1)


def test_screen_partition(vr, gpu, golden, oracle, volumes, tf):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole frame, RGBA and
    depth; depth rows beyond the view hold -1"""
    vox = volumes["blob_40x24x56"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(120, 72, 5)          # 72 rows: rank 1's second band (rows 64..79) ends beyond the view
    for sampling in SAMPLINGS:
        ref, ref_depth, counters = expected(vr, oracle, vox, view, sampling, tf, 100.0)
        assert counters["hits"] > 500
        p, per_rank = vr.band_partition(frame_params(vr, oracle, vox, view, sampling, 1), 1, 3, 16)
        assert (p.band_rows, p.band_stride, p.band_first) == (16, 3, 1)
        out, depth = gpu.render_iso(p, 100.0, REFINE, depth=True)
        assert out.shape[0] == per_rank * 16 and depth.shape == out.shape[:2]
        want = expected_bands(ref, 1, 3, 16, per_rank * 16)
        assert np.array_equal(out, want), (sampling, np.flatnonzero((out != want).any(axis=(1, 2))))      # (the local rows that differ)
        assert depth_diff(depth, expected_bands(ref_depth, 1, 3, 16, per_rank * 16, beyond=-1)) == 0, sampling
        assert (~expected_bands(np.ones(72, bool), 1, 3, 16, per_rank * 16)).sum() == 8                     # rows beyond the view
        p = frame_params(vr, oracle, vox, view, sampling, 1)
        p.x0, p.out_width = 24, 40
        out, depth = gpu.render_iso(p, 100.0, REFINE, depth=True)
        assert np.array_equal(out, ref[:, 24:64]) and np.array_equal(depth_bits(depth), depth_bits(ref_depth[:, 24:64])), sampling


def test_entry_points_and_error_conventions(vr, gpu, golden, oracle, volumes, tf):
    import torch
    vox = volumes["bucky"]
    load(gpu, vox, tf)
    view = vr.benchmark_view(120, 72, 3)
    p = frame_params(vr, oracle, vox, view, 1, 1)
    ref = expected(vr, oracle, vox, view, 1, tf, 100.0)
    assert ref[2]["hits"] > 1000
    host, host_depth = check(gpu, p, 100.0, ref, "host")
    assert np.array_equal(gpu.render_iso(p, 100.0, REFINE), host)             # the same RGBA without a depth buffer
    buf = torch.full((72, 120, 4), 77, dtype=torch.uint8, device="cuda")
    dbuf = torch.full((72, 120), 123.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                            # (the fills run on torch's stream, the frame on the context's)
    gpu.timing_reset()
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        gpu.render_iso_device(p, 100.0, REFINE, buf.data_ptr(), dbuf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 3                      # one launch per device-pointer frame, counted by vr_hip_timing
    assert np.array_equal(buf.cpu().numpy(), host) and depth_diff(dbuf.cpu().numpy(), host_depth) == 0
    buf.fill_(77)
    dbuf.fill_(123.0)
    torch.cuda.synchronize()                            # (the fills run on torch's stream, the frame on the context's)
    gpu.render_iso_device(p, 100.0, REFINE, buf.data_ptr(), None, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), host) and bool((dbuf == 123.0).all())
    info = gpu.last_launch()
    assert info["tiles_x"] == 4 and info["tiles_y"] >= 5 and info["layout"] in (1, 5)
    L = vr.lib()
    iso = vr.VrIso(100.0, REFINE)
    assert L.vr_hip_render_iso(gpu._ctx, None, C.byref(iso), host.ctypes.data, None) == 1              # VR_ERR_INVALID, like vr_hip_render_mip
    assert L.vr_hip_render_iso(gpu._ctx, C.byref(p), None, host.ctypes.data, None) == 1
    assert L.vr_hip_render_iso(gpu._ctx, C.byref(p), C.byref(iso), None, None) == 1
    assert L.vr_hip_render_iso_device(gpu._ctx, C.byref(p), C.byref(iso), None, None, None) == 1
    assert L.vr_hip_render_iso_device(gpu._ctx, C.byref(p), None, buf.data_ptr(), None, None) == 1
    nearest = p.copy()
    nearest.sampling = 0
    with pytest.raises(vr.VrError) as e:
        gpu.render_iso(nearest, 100.0)
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    for level, refine in ((float("nan"), 4), (float("inf"), 4), (100.0, 17)):
        with pytest.raises(vr.VrError) as e:
            gpu.render_iso(p, level, refine)
        assert e.value.code == 1, (level, refine)
    fresh = vr.HipRenderer(0)
    try:
        fresh.set_window_buffer(128, 128)
        with pytest.raises(vr.VrError) as e:
            fresh.render_iso(p, 100.0)
        assert e.value.code == 5                           # VR_ERR_NOT_READY: no volume
        fresh.set_volume(vox)
        with pytest.raises(vr.VrError) as e:
            fresh.render_iso(p, 100.0)
        assert e.value.code == 5                           # ... no transfer function
        fresh.set_transfer_fn(tf, np.zeros(1024, np.uint32))
        check(fresh, p, 100.0, ref, "fresh")
    finally:
        fresh.close()


def test_other_modes_are_unchanged_around_iso_frames(vr, gpu, golden, oracle, volumes):
    """A composite frame and a MIP frame rendered before and after isosurface frames on the same context"""
    case = next(c for c in golden.cases(True) if c["label"] == "bench64_view5_default")
    st = golden.volume_state("bucky")
    vox = volumes["bucky"]
    gpu.set_window_buffer(128, 128)
    gpu.set_transfer_fn(st["tf"], st["esl"])
    gpu.set_volume(vox)
    for sampling in SAMPLINGS:
        p = golden.params(case, sampling)
        before, mip_before = gpu.render_volume(p), gpu.render_mip(p)
        assert diff(mip_before, MipRef.instance().render(p, vox, st["tf"])[0]) == 0
        for esl in (0, 1):
            q = p.copy()
            q.esl = esl
            ref = IsoRef.instance().render(golden.params(case, sampling), vox, st["tf"], 100.0, REFINE)
            assert ref[2]["hits"] > 500
            check(gpu, q, 100.0, ref, (sampling, esl))
        assert np.array_equal(gpu.render_volume(p), before) and np.array_equal(gpu.render_mip(p), mip_before), sampling


def test_a_new_volume_brings_its_own_block_maxima(vr, gpu, golden, oracle, volumes, tf):
    """Volume A, then B on the same context: B's frames skip by B's maxima (A is bright where B is empty and the other way round)"""
    a, b = volumes["first_slice"], volumes["corner"]
    view = vr.benchmark_view(80, 80, 1)
    load(gpu, a, tf)
    for sampling in SAMPLINGS:
        check(gpu, frame_params(vr, oracle, a, view, sampling, 1), 24.5, expected(vr, oracle, a, view, sampling, tf, 24.5), ("a", sampling))
    gpu.set_volume(b)
    hits = 0
    for sampling in SAMPLINGS:
        ref = expected(vr, oracle, b, view, sampling, tf, 24.5)
        hits += ref[2]["hits"]
        check(gpu, frame_params(vr, oracle, b, view, sampling, 1), 24.5, ref, ("b", sampling))
    assert hits > 0


def test_release_linear_copy_keeps_skipping_frames_possible(vr, golden, oracle, volumes, tf):
    """The block maxima are scanned from the linear array: vr_hip_release_linear_copy derives them before it frees it"""
    vox = volumes["late_max"]
    view = vr.benchmark_view(80, 80, 6)
    r = vr.HipRenderer(0)
    try:
        load(r, vox, tf)
        ref = expected(vr, oracle, vox, view, 1, tf, 24.5)
        assert ref[2]["hits"] > 1000
        check(r, frame_params(vr, oracle, vox, view, 1, 0), 24.5, ref, "esl off")      # builds the quad bricks, not the block maxima
        r.release_linear_copy()
        assert r.volume_info().linear_resident == 0
        check(r, frame_params(vr, oracle, vox, view, 1, 1), 24.5, ref, "esl on, released")
    finally:
        r.close()


def test_driver_iso_flag(golden, tmp_path):
    """volr_bench -iso (HipRenderer::set_iso through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at distance 2"""
    out, rgb = run_driver(tmp_path, "-iso", "100", "-refine", "4")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Isosurface" in out.stdout
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    ref = IsoRef.instance().render(golden.params(case, 1), np.ascontiguousarray(golden.voxels("bucky")), golden.volume_state("bucky")["tf"], 100.0, 4)
    assert ref[2]["hits"] > 5000
    assert np.array_equal(rgb, ref[0][..., :3])
    out, _ = run_driver(tmp_path, "-iso", "100", "-devices", "0,0", size=(128, 128), pose=None, renderer=None, output=None)
    assert out.returncode != 0 and "single device" in out.stdout
