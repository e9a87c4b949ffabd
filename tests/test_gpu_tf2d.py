"""GPU tier of the 2D transfer-function frames (vr_hip_set_tf2d, vr_hip_render_tf2d*, vr_hip_gradient_histogram): every frame the tf2d_kernel
family renders is held byte for byte, no tolerance anywhere, against tf2d_render of tests/tf2d_ref.c, the contract of include/vr_hip.h
restated with the CPU oracle's statics, and every histogram count against gradient_histogram_ref.  tests/test_tf2d_model.py ties those
restatements to the composite restatements and to a numpy statement, and shows that the frames compared here reach every row pair and both
kinds of entry and tell four wrong readings of the contract apart."""
import ctypes as C
import importlib

import numpy as np
import pytest

import feature_random as fr
from clip_helpers import CLIPS
from gpu_feature import PATH_VOLUMES, diff, expected_bands, load, needs_bounds_lib, reset_context, run_under_bounds_build, sweep_paths
from label_helpers import Case, random_case, set_state, tier_frames
from light_helpers import LIT_VOLUMES, PHONG, lit_views, lit_volumes
from slab_helpers import slab_scene
from tf2d_helpers import Tf2dRef, check, choose_g_scale, equal_rows, esl_of, random_table, structured_table, tf2d_launch

pytestmark = pytest.mark.gpu

TF2D_STREAM = 10                                        # the generator stream of the random scenes (0-9 are taken by the other feature files)
RANDOM_WINDOW = (70, 50)


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(scope="module")
def gpu(vr):
    """a Tf2dRenderer of this module's own on cuda:0, closed at the end"""
    import torch  # noqa: F401  (loads the process's HIP runtime first)
    r = importlib.import_module("volume-rendering_amd.tf2d").Tf2dRenderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole module: no test leaves a state, a layout, a forced path or a table behind"""
    yield
    reset_context(vr, gpu)
    gpu.clear_tf2d()


def plain_case(vr, golden, oracle, volumes, name, view, sampling, full_march, **kw):
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
    settings = dict(what=(name, sampling), vox=vox, p=p, tf=tf, esl=esl, clip=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0)), set_clip=None, lighting=None,
                    q=None, shadow=None, strength=1.0)
    settings.update(kw)
    return Case(**settings)


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", LIT_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """The list of label_helpers.tier_frames — nine views, two frames each: the cue, the lighting, the shadow and both; no clip, box, plane
    and both; the default mode and the full march; the ray step and four times it — with the structured table of the volume's own function,
    the volume's g_scale and the leaping bits of the envelope: bytes, one frame counted each"""
    ref = Tf2dRef.instance()
    g_scale = choose_g_scale(name, volumes[name])
    loaded = False
    frames = pixels = 0
    start = gpu.tf2d_frames()
    for case in tier_frames(vr, golden, oracle, volumes, name, sampling):
        table = structured_table(case.tf)
        bits = esl_of(oracle, case.vox, table)
        if not loaded:
            load(gpu, case.vox, case.tf, case.esl)
            gpu.set_tf2d(table, g_scale, bits)
            loaded = True
        set_state(gpu, case)
        want = check(gpu, ref, case, table, g_scale, bits)
        frames, pixels = frames + 1, pixels + int(want.frame[..., 3].astype(bool).sum())
    print(f"{name} sampling {sampling}: {frames} frames, {pixels} pixels with alpha compared")
    assert frames == 18 and pixels > 18 * 200 and gpu.tf2d_frames() == start + frames, (frames, pixels)


def test_consequences_on_the_device(vr, gpu, golden, oracle, volumes):
    """(a) every row the context's transfer function, with its ESL bits, two values of g_scale: the bytes of render_volume under the same
    clip, lighting and shadow; (b) g_scale = 0 with the structured table: the bytes of render_volume with row 0 as the function and the
    envelope's bits (no shadow: the light grid follows the 1-D function); (d) an all-zero table: all zero bytes — on the device alone, over
    frames of the four volumes' lists: the cue, the lighting, the shadow and both, clipped and not"""
    compared = flat = 0
    kinds = set()
    for name in LIT_VOLUMES:
        loaded = False
        for k, case in enumerate(list(tier_frames(vr, golden, oracle, volumes, name, 1))[::3]):
            if not loaded:
                load(gpu, case.vox, case.tf, case.esl)
                loaded = True
            else:
                gpu.set_transfer_fn(case.tf, case.esl)
            set_state(gpu, case)
            kinds.add((case.lighting is not None, case.q is not None, case.set_clip is not None))
            plain = gpu.render_volume(case.p)
            for g_scale in (0.37 * (k + 1), 1e30):
                gpu.set_tf2d(equal_rows(case.tf, 2 + k % 7), g_scale, case.esl)
                got = gpu.render_tf2d(case.p)
                assert diff(got, plain) == 0, (case.what, "a", g_scale, diff(got, plain))
            gpu.set_tf2d(np.zeros((2, 128, 4), np.float32), 1.0, np.zeros(1024, np.uint32))
            assert not gpu.render_tf2d(case.p).any(), (case.what, "d")
            compared += int(plain[..., 3].astype(bool).sum())
            if case.q is None:
                table = structured_table(case.tf)
                bits = esl_of(oracle, case.vox, table)
                gpu.set_tf2d(table, 0.0, bits)
                got = gpu.render_tf2d(case.p)
                gpu.set_transfer_fn(table[0], bits)
                want = gpu.render_volume(case.p)
                assert diff(got, want) == 0, (case.what, "b", diff(got, want))
                flat += int(want[..., 3].astype(bool).sum())
    assert compared > 24 * 200 and flat > 8 * 200, (compared, flat)
    assert {k[:2] for k in kinds} == {(False, False), (True, False), (False, True), (True, True)} and {k[2] for k in kinds} == {False, True}, kinds


def test_every_path_agrees(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / 4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, never a run copy or a column window, never a measured order; u8
    and u16 (oct bricks), the structured table; a lit frame of the default mode and a clipped frame of the full march with the cue"""
    ref = Tf2dRef.instance()
    for name, expect in PATH_VOLUMES:
        views = [v for v in lit_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for k, (label, view) in enumerate(views):
            cases.append(plain_case(vr, golden, oracle, volumes, name, view, 1 + k % 2, False, what=(name, label, "lit"), lighting=PHONG))
            cases.append(plain_case(vr, golden, oracle, volumes, name, view, 1 + k % 2, True, what=(name, label, "cue"), set_clip=CLIPS["both"], clip=CLIPS["both"]))
        vox = cases[0].vox
        table = structured_table(cases[0].tf)
        bits = esl_of(oracle, vox, table)
        g_scale = choose_g_scale(name, vox)
        load(gpu, vox, cases[0].tf, cases[0].esl)
        gpu.set_tf2d(table, g_scale, bits)
        seen = set()

        def check_all(what):
            for case in cases:
                set_state(gpu, case)
                case.what = case.what[:3] + (what,)
                check(gpu, ref, case, table, g_scale, bits)
                seen.add(gpu.last_launch()["layout"])
        sweep_paths(vr, gpu, check_all)
        assert seen == expect, (name, seen)


def test_bands_crop_and_device_entry_point(vr, gpu, golden, oracle, volumes):
    """Three ranks of interleaved 16-row bands (a view of 70 rows: 5 bands, so two ranks hold a band beyond the view, which is zero) and a
    crop in x equal the matching rows / columns of the whole frame; the device entry point renders the same in one launch into a torch
    buffer on a torch stream"""
    import torch
    name = "blob_40x24x56"
    ref = Tf2dRef.instance()
    case = plain_case(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 70, 5), 1, False, lighting=PHONG)
    table = structured_table(case.tf)
    bits = esl_of(oracle, case.vox, table)
    g_scale = choose_g_scale(name, case.vox)
    load(gpu, case.vox, case.tf, case.esl)
    gpu.set_tf2d(table, g_scale, bits)
    set_state(gpu, case)
    whole = case.p
    want = check(gpu, ref, case, table, g_scale, bits).frame
    assert want[..., 3].astype(bool).sum() > 1000
    for rank in range(3):
        p, per_rank = vr.band_partition(whole.copy(), rank, 3, 16)
        rows = per_rank * 16
        assert p.out_rows == rows == 32
        assert diff(gpu.render_tf2d(p), expected_bands(want, rank, 3, 16, rows)) == 0, rank
    crop = whole.copy()
    crop.x0, crop.out_width = 24, 40
    assert diff(gpu.render_tf2d(crop), want[:, 24:64]) == 0
    frame = torch.full((70, 120, 4), 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                            # (the fill runs on torch's stream, the frame on the context's)
    gpu.timing_reset()
    before = gpu.tf2d_frames()
    gpu.render_tf2d_device(whole, frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and gpu.tf2d_frames() == before + 1 and tf2d_launch(gpu.last_launch())
    assert diff(frame.cpu().numpy(), want) == 0


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65: clamped differences on both sides, brick edges, ragged last
    bricks, the table pad) from views 0, 1 and 5 at 48 x 40 (no multiple of the tile) under both clips of its frames, with their esl and
    thresholds, the structured table, the shading cycling through the cue, the lighting, the shadow and both"""
    ref = Tf2dRef.instance()
    gpu.set_window_buffer(*fr.EDGE_SIZE)
    frames = 0
    for i, shape in enumerate(fr.EDGE_SHAPES):
        s = fr.edge_scene(oracle, vr, shape, dtype)
        table = structured_table(s.tf)
        bits = esl_of(oracle, s.vox, table)
        g_scale = 2.0 ** -7 if dtype == "uint8" else 2.0 ** -15
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        gpu.set_tf2d(table, g_scale, bits)
        for j, f in enumerate(s.frames):
            case = random_case(s, j, f, (i + j) % 4)
            case.what = (shape, dtype, f.view, f.clip_name) + case.what[3:4]
            set_state(gpu, case)
            check(gpu, ref, case, table, g_scale, bits)
            frames += 1
    assert frames == len(fr.EDGE_SHAPES) * len(fr.EDGE_VIEWS) * len(fr.EDGE_CLIPS)


@pytest.mark.parametrize("which", ("random", "holed"))
def test_random_frames(vr, gpu, oracle, which):
    """The random frames and the holed scenes of tests/feature_random.py under their own clip, lighting and shadow, layout and wide addressing
    alternating per scene, each scene with a table of 2 to 8 rows and a g_scale drawn from a stream of its own"""
    ref = Tf2dRef.instance()
    scenes = fr.random_scenes(oracle, vr, TF2D_STREAM) if which == "random" else fr.holed_scenes(oracle, vr)
    rng = np.random.default_rng([fr.SEED, TF2D_STREAM, 0 if which == "random" else 1])
    frames = pixels = 0
    rows = set()
    start = gpu.tf2d_frames()
    for s, scene in enumerate(scenes):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene.vox, scene.tf, scene.esl, RANDOM_WINDOW)
        table = random_table(rng, scene.tf)
        bits = esl_of(oracle, scene.vox, table)
        top = float(np.iinfo(scene.vox.dtype).max) * 0.5 * max(scene.vox.shape)
        g_scale = float(np.float32(table.shape[0] * rng.uniform(1.0, 8.0) / top))
        gpu.set_tf2d(table, g_scale, bits)
        rows.add(table.shape[0])
        for i, f in enumerate(scene.frames):
            case = random_case(scene, i, f, (s + i) % 4)
            case.what = case.what + ("layout", scene.layout, "wide", scene.wide, "rows", table.shape[0])
            set_state(gpu, case)
            want = check(gpu, ref, case, table, g_scale, bits)
            frames, pixels = frames + 1, pixels + int(want.frame[..., 3].astype(bool).sum())
    print(f"{which}: {frames} frames, {pixels} pixels with alpha compared, rows {sorted(rows)}")
    assert frames == sum(len(s.frames) for s in scenes) and pixels > 20 * frames and gpu.tf2d_frames() == start + frames, (frames, pixels)


def test_state(vr, gpu, golden, oracle, volumes):
    """A frame without a table, every error of step 11, the table surviving set_volume, set_transfer_fn and set_labels not changing a tf2d
    frame, and what a table leaves alone: the composite, labelled, MIP and depth frames keep their bytes"""
    import torch
    ref = Tf2dRef.instance()
    case = plain_case(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(128, 128, 1), 1, False)
    vox, p = case.vox, case.p
    load(gpu, vox, case.tf, case.esl)
    labels = ((np.arange(vox.size, dtype=np.uint32).reshape(vox.shape) // 7) % 5).astype(np.uint8)
    gpu.set_labels(labels)
    gpu.set_label_table([vr.binding.make_label_entry((1.0, 0.0, 0.0), 0.5, 0.75)] * 3)
    others = (gpu.render_volume(p), gpu.render_labelled(p), gpu.render_mip(p), gpu.render_depth(p, 0.5))
    L = vr.lib()
    out = np.zeros((p.out_rows, p.out_width, 4), np.uint8)
    dev = torch.zeros((p.out_rows, p.out_width, 4), dtype=torch.uint8, device="cuda")

    def refused(params):
        return [L.vr_hip_render_tf2d(gpu._ctx, C.byref(params), out.ctypes.data), L.vr_hip_render_tf2d_device(gpu._ctx, C.byref(params), dev.data_ptr(), None)]
    count = gpu.tf2d_frames()
    assert refused(p) == [5, 5]                         # VR_ERR_NOT_READY: no table yet
    table = structured_table(case.tf)
    bits = esl_of(oracle, vox, table)
    g_scale = choose_g_scale("bucky", vox)

    def set_raw(t, rows, scale, esl):
        return L.vr_hip_set_tf2d(gpu._ctx, t.ctypes.data, rows, scale, None if esl is None else esl.ctypes.data)
    big = np.zeros((9, 128, 4), np.float32)
    nan, inf = float("nan"), float("inf")
    assert set_raw(big, 1, 1.0, bits) == 1 and set_raw(big, 9, 1.0, bits) == 1 and set_raw(big, 0, 1.0, bits) == 1
    assert [set_raw(big, 2, v, bits) for v in (nan, inf, -inf, -1.0)] == [1, 1, 1, 1]
    assert set_raw(big, 2, 1.0, None) == 1
    for value in (nan, inf, -inf, -0.25):
        bad = np.array(table)
        bad[3, 77, 2] = value
        assert set_raw(bad, 5, 1.0, bits) == 1, value
    assert refused(p) == [5, 5]                         # a refused table sets none
    gpu.set_tf2d(table, g_scale, bits)
    want = check(gpu, ref, case, table, g_scale, bits).frame
    assert set_raw(big, 9, 1.0, bits) == 1              # a refused table leaves the one before in place
    assert diff(gpu.render_tf2d(p), want) == 0
    nearest = p.copy()
    nearest.sampling = 0
    assert refused(nearest) == [1, 1]
    with pytest.raises(vr.VrError) as e:
        gpu.render_tf2d(nearest)
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    gpu.set_preintegration()
    assert refused(p) == [1, 1]
    gpu.clear_preintegration()
    assert L.vr_hip_render_tf2d(gpu._ctx, C.byref(p), None) == 1 and L.vr_hip_render_tf2d_device(gpu._ctx, None, dev.data_ptr(), None) == 1
    assert L.vr_hip_tf2d_frames(gpu._ctx, None) == 1
    hist = np.zeros((33, 256), np.uint64)
    assert [L.vr_hip_gradient_histogram(gpu._ctx, n, 1.0, hist.ctypes.data, None) for n in (0, 33)] == [1, 1]
    assert [L.vr_hip_gradient_histogram(gpu._ctx, 4, v, hist.ctypes.data, None) for v in (nan, inf, -1.0)] == [1, 1, 1]
    assert L.vr_hip_gradient_histogram(gpu._ctx, 4, 1.0, None, None) == 1
    assert gpu.tf2d_frames() == count + 2
    # what the table leaves alone, and what leaves the table alone
    again = (gpu.render_volume(p), gpu.render_labelled(p), gpu.render_mip(p), gpu.render_depth(p, 0.5))
    for x, y in zip(others, again):
        assert np.array_equal(x, y)
    gpu.set_transfer_fn(np.asarray(case.tf, np.float32) * np.float32(0.5), np.zeros(1024, np.uint32))
    gpu.set_labels(np.zeros(vox.shape, np.uint8))
    gpu.set_label_table(None)
    assert diff(gpu.render_tf2d(p), want) == 0
    gpu.set_volume(vox)                                 # a new volume drops the labels; the table stays
    assert diff(gpu.render_tf2d(p), want) == 0
    gpu.clear_tf2d()
    assert refused(p) == [5, 5] and gpu.tf2d_frames() == count + 4


def test_gradient_histogram(vr, gpu, golden, oracle, volumes):
    """vr_hip_gradient_histogram against gradient_histogram_ref on the edge shapes x dtypes (extents of 1 and 2: clamped on both sides; lines
    of 1 to 65 voxels, 1 to 527 lines: more lines than workgroups and fewer), the blob and bucky, with 1, 5 and 32 rows: every count; the sum
    over the rows is volume_histogram()"""
    ref = Tf2dRef.instance()
    cases = [("bucky", volumes["bucky"], choose_g_scale("bucky", volumes["bucky"])),
             ("blob", volumes["blob_40x24x56"], choose_g_scale("blob_40x24x56", volumes["blob_40x24x56"]))]
    for shape in fr.EDGE_SHAPES:
        for dtype in fr.EDGE_DTYPES:
            cases.append(((shape, dtype), fr.edge_volume(shape, dtype), 2.0 ** -7 if dtype == "uint8" else 2.0 ** -15))
    checked = 0
    for what, vox, g_scale in cases:
        gpu.set_volume(vox)
        plain = gpu.volume_histogram()[0]
        for g_bins in (1, 5, 32):
            scale = float(np.float32(g_scale * g_bins / 5.0))
            got = gpu.gradient_histogram(g_bins, scale)
            want = ref.histogram(vox, g_bins, scale)
            assert got.shape == (g_bins, 256) and np.array_equal(got, want), (what, g_bins, int((got != want).sum()))
            assert np.array_equal(got.sum(axis=0), plain), (what, g_bins)
            checked += 1
    assert checked == 3 * (2 + len(fr.EDGE_SHAPES) * len(fr.EDGE_DTYPES)) and gpu.last_gradient_histogram_ms > 0


@needs_bounds_lib
def test_tf2d_frames_under_the_bounds_checked_build():
    """A subset of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): the main list of one
    volume, the edge shapes and the histogram — every gather address of the frames and every load of the histogram is held against its
    array: a violation fails the call (VrError), and the bytes and counts still equal the restatements"""
    run_under_bounds_build(__file__, "edge_shapes or gradient_histogram or (frames_equal and random_u16)", 5, timeout=900)
