"""GPU tier of the clip region (vr_hip_set_clip / vr_hip_multi_set_clip): every clipped frame the HIP path renders — composite, MIP,
isosurface with depth — is held byte for byte / bit for bit against the clip_* entry points of tests/feature_ref.c, the three projections
restated with the CPU oracle's statics and the segment of every ray narrowed as include/vr_hip.h defines it.  tests/test_clip_model.py ties that restatement to the pinned
ones and shows that the frames compared here are neither empty nor unclipped."""
import ctypes as C

import numpy as np
import pytest

from clip_helpers import BOTH, BOX, CLIPS, IDENTITY, NOTHING, PLANE, ClipRef, composite_params, parallel_plane, set_clip
from gpu_feature import assert_order_repeats, depth_diff, diff, expected_bands, load, multi_pair, reset_context, run_driver, sweep_paths
from iso_helpers import PAIRS, all_volumes, depth_bits, frame_params, views_for
from mip_helpers import ramp_tf

pytestmark = pytest.mark.gpu

COMPOSITE_VOLUMES = ("bucky", "blob_40x24x56", "random_u16")
PROJECTION_VOLUMES = ("late_max", "corner", "blob_40x24x56", "random_u16")
LEVELS = {name: [level for n, level in PAIRS if n == name] for name in PROJECTION_VOLUMES}
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


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
@pytest.mark.parametrize("name", COMPOSITE_VOLUMES)
def test_composite_equals_the_restatement(vr, gpu, golden, oracle, volumes, name, clip_name):
    """Nine views x {NEAREST, TRILINEAR, Q8} x {default mode: leaping + early termination, full march}, lit"""
    vox, clip, ref = volumes[name], CLIPS[clip_name], ClipRef.instance()
    loaded = False
    for label, view in views_for(vr, golden, name):
        for sampling in (0, 1, 2):
            for full_march in (False, True):
                p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, sampling, full_march)
                if not loaded:
                    load(gpu, vox, ctf, esl)
                    set_clip(gpu, clip)
                    loaded = True
                out = gpu.render_volume(p)
                want = ref.composite(p, vox, ctf, esl, clip)
                assert diff(out, want) == 0, (name, clip_name, label, sampling, full_march, diff(out, want))
                assert gpu.last_launch()["layout"] not in (2, 3, 6, 7)


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
@pytest.mark.parametrize("name", PROJECTION_VOLUMES)
def test_mip_and_isosurface_equal_the_restatement(vr, gpu, golden, oracle, volumes, tf, name, clip_name):
    """MIP at the three samplings, isosurface with depth at the two TRILINEAR ones and the levels of PAIRS, esl off and on"""
    vox, clip, ref = volumes[name], CLIPS[clip_name], ClipRef.instance()
    load(gpu, vox, tf)
    set_clip(gpu, clip)
    for label, view in views_for(vr, golden, name):
        for sampling in (0, 1, 2):
            want = ref.mip(frame_params(vr, oracle, vox, view, sampling, 0), vox, tf, clip)
            for esl in (0, 1):
                out = gpu.render_mip(frame_params(vr, oracle, vox, view, sampling, esl))
                assert diff(out, want) == 0, (name, clip_name, label, "mip", sampling, esl, diff(out, want))
            if sampling == 0:
                continue
            for level in LEVELS[name]:
                want, want_depth, _ = ref.iso(frame_params(vr, oracle, vox, view, sampling, 0), vox, tf, level, REFINE, clip)
                for esl in (0, 1):
                    out, depth = gpu.render_iso(frame_params(vr, oracle, vox, view, sampling, esl), level, REFINE, depth=True)
                    assert diff(out, want) == 0 and depth_diff(depth, want_depth) == 0, (name, clip_name, label, "iso", level, sampling, esl,
                                                                                        diff(out, want), depth_diff(depth, want_depth))


def _three_modes(vr, gpu, oracle, vox, view, ctf_params, sampling=1):
    """(composite, mip, iso frame, iso depth) of one view; ctf_params: the composite's parameters"""
    q = frame_params(vr, oracle, vox, view, sampling, 1)
    iso, depth = gpu.render_iso(q, 100.0, REFINE, depth=True)
    return gpu.render_volume(ctf_params), gpu.render_mip(q), iso, depth


def test_identity_nothing_and_parallel(vr, gpu, golden, oracle, volumes):
    """IDENTITY equals the frame rendered with clipping off, NOTHING leaves zeros and depth -1, PARALLEL (n . direction exactly 0 on the
    orthogonal view 0: whole rays are kept or missed) equals the restatement — all three projections"""
    name = "bucky"
    vox, ref = volumes[name], ClipRef.instance()
    kept = 0
    for i, (label, view) in enumerate(views_for(vr, golden, name)):
        p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, 1, False)
        if i == 0:
            load(gpu, vox, ctf, esl)
        gpu.clear_clip()
        plain = _three_modes(vr, gpu, oracle, vox, view, p)
        set_clip(gpu, IDENTITY)
        same = _three_modes(vr, gpu, oracle, vox, view, p)
        assert all(np.array_equal(a, b) for a, b in zip(plain[:3], same[:3])) and depth_diff(plain[3], same[3]) == 0, label
        set_clip(gpu, NOTHING)
        none = _three_modes(vr, gpu, oracle, vox, view, p)
        assert not none[0].any() and not none[1].any() and not none[2].any() and (none[3] == -1).all(), label
        if label == "view0":
            clip = parallel_plane(view)
            set_clip(gpu, clip)
            got = _three_modes(vr, gpu, oracle, vox, view, p)
            q = frame_params(vr, oracle, vox, view, 1, 0)
            want_iso = ref.iso(q, vox, ctf, 100.0, REFINE, clip)
            assert diff(got[0], ref.composite(p, vox, ctf, esl, clip)) == 0 and diff(got[1], ref.mip(q, vox, ctf, clip)) == 0
            assert diff(got[2], want_iso[0]) == 0 and depth_diff(got[3], want_iso[1]) == 0
            kept = int(got[1].any(axis=-1).sum())
            assert 0 < kept < int(plain[1].any(axis=-1).sum())
    assert kept > 0


def test_axis_aligned_views_leave_the_column_march_and_return_to_it(vr, gpu, golden, oracle, volumes):
    """Orthogonal full-march TRILINEAR views 0 / 2 / 3: the column march (layout 7) where it is taken today, a quad / linear / oct copy
    under BOX with the restatement's bytes, and the column march and the first frame again after clear_clip()"""
    name = "bucky"
    vox, ref = volumes[name], ClipRef.instance()
    columns = 0
    for i in (0, 2, 3):
        view = vr.benchmark_view(80, 80, i)
        p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, 1, True)
        if i == 0:
            load(gpu, vox, ctf, esl)
        gpu.clear_clip()
        first = gpu.render_volume(p)
        before = gpu.last_launch()["layout"]
        columns += before == 7
        assert diff(first, ref.composite(p, vox, ctf, esl, IDENTITY)) == 0, i
        set_clip(gpu, BOX)
        assert diff(gpu.render_volume(p), ref.composite(p, vox, ctf, esl, BOX)) == 0, i
        assert gpu.last_launch()["layout"] in (0, 1, 5), (i, gpu.last_launch())
        gpu.clear_clip()
        assert np.array_equal(gpu.render_volume(p), first) and gpu.last_launch()["layout"] == before, i
    assert columns == 3, columns


def test_every_path_agrees_under_both(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / +4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, and never a run copy or a column window"""
    name = "blob_40x24x56"
    vox, ref = volumes[name], ClipRef.instance()
    views = [v for v in views_for(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
    cases = []
    for label, view in views:
        for sampling in (0, 1):
            p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, sampling, True)
            cases.append((label, sampling, p, ref.composite(p, vox, ctf, esl, BOTH)))
    load(gpu, vox, ctf, esl)
    set_clip(gpu, BOTH)
    seen = set()

    def check(what):
        for label, sampling, p, want in cases:
            out = gpu.render_volume(p)
            info = gpu.last_launch()
            assert diff(out, want) == 0, (what, label, sampling, diff(out, want), info)
            assert info["layout"] not in (2, 3, 6, 7), (what, label, sampling, info)
            seen.add(info["layout"])
    sweep_paths(vr, gpu, check)
    assert seen == {0, 1, 4}, seen              # linear array, quad bricks, voxel bricks (NEAREST)


def test_tile_scheduling_repeats_and_a_second_clip(vr, gpu, golden, oracle, volumes):
    """Default mode under the measured-cost tile order: the same clipped parameters four times give equal frames (estimate, recordings,
    recorded order), then another clip with the same vr_params — the caches are keyed by them alone — equals its own restatement"""
    name = "bucky"
    vox, ref = volumes[name], ClipRef.instance()
    view = vr.benchmark_view(256, 256, 1)                      # 8 x 16 workgroup tiles: the tile order is kept for 64 tiles and more
    p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, 1, False)
    load(gpu, vox, ctf, esl)
    gpu.set_window_buffer(256, 256)
    gpu.set_tile_scheduling(1)
    for clip in (BOX, PLANE):
        set_clip(gpu, clip)
        want = ref.composite(p, vox, ctf, esl, clip)
        assert want.any()
        assert_order_repeats(gpu, lambda: gpu.render_volume(p), want, what=(clip,))


def test_screen_partition(vr, gpu, golden, oracle, volumes, tf):
    """Interleaved bands (rank 1 of 3, 16 rows each) and a crop in x equal the matching rows / columns of the whole clipped frame,
    composite and isosurface with depth"""
    name = "blob_40x24x56"
    vox, ref = volumes[name], ClipRef.instance()
    view = vr.benchmark_view(120, 72, 5)
    load(gpu, vox, tf)
    set_clip(gpu, BOTH)
    whole = frame_params(vr, oracle, vox, view, 1, 1)
    whole.ray_threshold = 1.0
    unskipped = frame_params(vr, oracle, vox, view, 1, 0)
    unskipped.ray_threshold = 1.0
    want_dvr = ref.composite(unskipped, vox, tf, np.zeros(1024, np.uint32), BOTH)
    want_iso, want_depth, _ = ref.iso(unskipped, vox, tf, 100.0, REFINE, BOTH)
    assert want_dvr.any() and (want_depth >= 0).sum() > 300
    p, per_rank = vr.band_partition(whole.copy(), 1, 3, 16)
    q = p.copy()
    q.esl = 0                                                   # (the composite would leap by the ESL bits, which are all zero here: nothing to leap)
    out_dvr = gpu.render_volume(q)
    out_iso, depth = gpu.render_iso(p, 100.0, REFINE, depth=True)
    rows = per_rank * 16
    assert out_dvr.shape[0] == rows
    for kind, got, whole_frame in (("composite", out_dvr, want_dvr), ("iso", out_iso, want_iso)):
        expected = expected_bands(whole_frame, 1, 3, 16, rows)
        assert np.array_equal(got, expected), (kind, np.flatnonzero((got != expected).any(axis=(1, 2))))      # (the local rows that differ)
    assert depth_diff(depth, expected_bands(want_depth, 1, 3, 16, rows, beyond=-1)) == 0
    crop = unskipped.copy()
    crop.x0, crop.out_width = 24, 40
    assert np.array_equal(gpu.render_volume(crop), want_dvr[:, 24:64])
    out_iso, depth = gpu.render_iso(crop, 100.0, REFINE, depth=True)
    assert np.array_equal(out_iso, want_iso[:, 24:64]) and np.array_equal(depth_bits(depth), depth_bits(want_depth[:, 24:64]))


def test_errors_and_entry_points(vr, gpu, golden, oracle, volumes, tf):
    import torch
    name = "bucky"
    vox, ref = volumes[name], ClipRef.instance()
    view = vr.benchmark_view(120, 72, 3)
    p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, 1, False)
    load(gpu, vox, ctf, esl)
    L = vr.lib()
    good = vr.VrClip((C.c_float * 3)(*BOTH[0]), (C.c_float * 3)(*BOTH[1]), (C.c_float * 4)(*BOTH[2]))
    assert L.vr_hip_set_clip(None, C.byref(good)) == 1
    for member, index in (("box_min", 1), ("box_max", 2), ("plane", 0), ("plane", 3)):
        for bad_value in (float("nan"), float("inf"), float("-inf")):
            bad = vr.VrClip.from_buffer_copy(good)
            getattr(bad, member)[index] = bad_value
            assert L.vr_hip_set_clip(gpu._ctx, C.byref(bad)) == 1, (member, index, bad_value)       # VR_ERR_INVALID
    for axis in range(3):
        for delta in (0.0, 0.5):
            bad = vr.VrClip.from_buffer_copy(good)
            bad.box_min[axis] = bad.box_max[axis] + delta
            assert L.vr_hip_set_clip(gpu._ctx, C.byref(bad)) == 1, (axis, delta)
    with pytest.raises(vr.VrError) as e:
        gpu.set_clip(box_min=(0.5, 0, 0), box_max=(0.5, 1, 1))
    assert e.value.code == 1 and "box_min" in str(e.value)
    plain = gpu.render_volume(p)                                # a refused clip changes nothing: still no clip
    assert diff(plain, ref.composite(p, vox, ctf, esl, IDENTITY)) == 0
    outside = vr.VrClip((C.c_float * 3)(2, 2, 2), (C.c_float * 3)(3, 3, 3), (C.c_float * 4)(0, 0, 0, 0))
    assert L.vr_hip_set_clip(gpu._ctx, C.byref(outside)) == 0   # a box that misses the cube is valid: an empty frame
    assert not gpu.render_volume(p).any()
    assert L.vr_hip_set_clip(gpu._ctx, C.byref(good)) == 0
    want = ref.composite(p, vox, ctf, esl, BOTH)
    assert want.any() and diff(gpu.render_volume(p), want) == 0
    assert L.vr_hip_set_clip(gpu._ctx, None) == 0               # NULL clears the clip
    assert np.array_equal(gpu.render_volume(p), plain)
    # device-pointer entry points on the caller's stream, one launch per frame
    set_clip(gpu, BOTH)
    q = frame_params(vr, oracle, vox, view, 1, 1)
    want_mip = ref.mip(frame_params(vr, oracle, vox, view, 1, 0), vox, ctf, BOTH)
    want_iso, want_depth, _ = ref.iso(frame_params(vr, oracle, vox, view, 1, 0), vox, ctf, 100.0, REFINE, BOTH)
    bufs = [torch.full((72, 120, 4), 77, dtype=torch.uint8, device="cuda") for _ in range(3)]
    dbuf = torch.full((72, 120), 123.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                            # (the fills run on torch's stream, the frame on the context's)
    gpu.timing_reset()
    gpu.render_volume_device(p, bufs[0].data_ptr(), stream)
    gpu.render_mip_device(q, bufs[1].data_ptr(), stream)
    gpu.render_iso_device(q, 100.0, REFINE, bufs[2].data_ptr(), dbuf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 3
    assert diff(bufs[0].cpu().numpy(), want) == 0 and diff(bufs[1].cpu().numpy(), want_mip) == 0
    assert diff(bufs[2].cpu().numpy(), want_iso) == 0 and depth_diff(dbuf.cpu().numpy(), want_depth) == 0


@pytest.mark.parametrize("transport", ("peer", "rccl-self"))
def test_multi_device_frames_are_clipped(vr, gpu, golden, oracle, volumes, monkeypatch, transport):
    """MultiRenderer([0, 0]).set_clip(BOTH) equals the single-device clipped frame (and so the restatement), by peer copies and through
    RCCL with one communicator"""
    name = "bucky"
    vox, ref = volumes[name], ClipRef.instance()
    view = vr.benchmark_view(120, 72, 5)
    with multi_pair(vr, monkeypatch, transport) as m:
        for sampling in (0, 1):
            p, ctf, esl = composite_params(vr, golden, oracle, name, vox, view, sampling, False)
            if sampling == 0:
                load(gpu, vox, ctf, esl)
                m.set_transfer_fn(ctf, esl)
                m.set_volume(vox)
            m.clear_clip()
            gpu.clear_clip()
            assert np.array_equal(m.render_volume(p), gpu.render_volume(p)), sampling
            set_clip(m, BOTH)
            set_clip(gpu, BOTH)
            single = gpu.render_volume(p)
            assert diff(single, ref.composite(p, vox, ctf, esl, BOTH)) == 0 and single.any()
            assert np.array_equal(m.render_volume(p), single), sampling
        with pytest.raises(vr.VrError) as e:
            m.set_clip(box_min=(0, 0, 0), box_max=(0, 1, 1))
        assert e.value.code == 1


def test_driver_clip_flags(golden, tmp_path):
    """volr_bench -clip-plane / -clip-box (HipRenderer::set_clip through the host mirror): Bucky.pvm, TRILINEAR, pose (-45,-45,0) at
    distance 2, 256 x 256 — the composite, and once more with -iso 100"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    for extra, expect in (([], lambda clip: ClipRef.instance().composite(p, vox, st["tf"], st["esl"], clip)),
                          (["-iso", "100"], lambda clip: ClipRef.instance().iso(p, vox, st["tf"], 100.0, 4, clip)[0])):
        for flags, clip in ((["-clip-plane"] + [repr(float(np.float32(v))) for v in PLANE[2]], PLANE),
                            (["-clip-box"] + [str(v) for v in BOX[0] + BOX[1]], BOX)):
            out, rgb = run_driver(tmp_path, *extra, *flags)
            assert out.returncode == 0, out.stdout + out.stderr
            assert "Clip region" in out.stdout
            want = expect(clip)
            assert want.any() and np.array_equal(rgb, want[..., :3]), (extra, flags)
    out, _ = run_driver(tmp_path, "-clip-box", "0", "0", "0", "0", "1", "1", size=(128, 128), pose=None, renderer=None)
    assert out.returncode != 0 and "box_min" in out.stdout
