"""GPU tier of the labelled composite frames (vr_hip_set_labels, vr_hip_set_label_table, vr_hip_render_labelled*): every frame the
label_kernel family renders is held byte for byte, no tolerance anywhere, against label_render of tests/label_ref.c, the contract of
include/vr_hip.h restated with the CPU oracle's statics.  tests/test_label_model.py ties that restatement to the composite restatements and
shows that the frames compared here reach every kind of table entry and tell four wrong readings of the contract apart."""
import ctypes as C

import numpy as np
import pytest

import feature_random as fr
from clip_helpers import CLIPS
from gpu_feature import PATH_VOLUMES, diff, expected_bands, load, needs_bounds_lib, reset_context, run_driver, run_under_bounds_build, sweep_paths
from label_helpers import (LABEL_VOLUMES, Case, LabelRef, check, constant_table, identity_table, label_launch, labels_for, random_case, random_labels, set_state,
                           structured_labels, table, tier_frames)
from light_helpers import PHONG, lit_views, lit_volumes
from slab_helpers import slab_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout, a forced path or labels behind"""
    yield
    reset_context(vr, gpu)
    gpu.set_label_table(None)


def plain_case(vr, golden, oracle, volumes, name, view, sampling, full_march, **kw):
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, full_march)
    settings = dict(what=(name, sampling), vox=vox, p=p, tf=tf, esl=esl, clip=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0)), set_clip=None, lighting=None,
                    q=None, shadow=None, strength=1.0)
    settings.update(kw)
    return Case(**settings)


@pytest.mark.parametrize("sampling", (1, 2))
@pytest.mark.parametrize("name", LABEL_VOLUMES)
def test_frames_equal_the_restatement(vr, gpu, golden, oracle, volumes, name, sampling):
    """The list of label_helpers.tier_frames — nine views, two frames each: the cue, the lighting, the shadow and both; no clip, box, plane
    and both; the default mode and the full march; the ray step and four times it — with the volume's labels (structured, random on the
    random volume) and the table of the five entry kinds: bytes, one frame counted each"""
    ref = LabelRef.instance()
    entries = table()
    loaded = False
    frames = pixels = 0
    start = gpu.labelled_frames()
    for case in tier_frames(vr, golden, oracle, volumes, name, sampling):
        if not loaded:
            load(gpu, case.vox, case.tf, case.esl)
            gpu.set_labels(labels_for(name, case.vox))
            gpu.set_label_table(entries)
            loaded = True
        set_state(gpu, case)
        want = check(gpu, ref, case, labels_for(name, case.vox), entries)
        frames, pixels = frames + 1, pixels + int(want.frame[..., 3].astype(bool).sum())
    print(f"{name} sampling {sampling}: {frames} frames, {pixels} pixels with alpha compared")
    assert frames == 18 and pixels > 18 * 200 and gpu.labelled_frames() == start + frames, (frames, pixels)


def test_consequences_on_the_device(vr, gpu, golden, oracle, volumes):
    """(a) an all-identity table: the bytes of render_volume under the same clip, lighting and shadow; (b) every opacity 0: all zero bytes;
    (c) one constant label with { mix 0, opacity 0.5 }, every other entry hidden, no shadow: the bytes of render_volume under the halved
    transfer function — on the device alone, over frames of the four volumes' lists"""
    hidden = constant_table(0.75, 0.0, (0.5, 0.25, 1.0))
    half = hidden.copy()
    half[7] = (0.0, 0.0, 0.0, 0.0, 0.5)
    compared = halved = 0
    for name in LABEL_VOLUMES:
        loaded = False
        for case in list(tier_frames(vr, golden, oracle, volumes, name, 1))[::3]:
            if not loaded:
                load(gpu, case.vox, case.tf, case.esl)
                loaded = True
            else:
                gpu.set_transfer_fn(case.tf, case.esl)
            gpu.set_labels(labels_for(name, case.vox))
            set_state(gpu, case)
            plain = gpu.render_volume(case.p)
            gpu.set_label_table(identity_table())
            got = gpu.render_labelled(case.p)
            assert diff(got, plain) == 0, (case.what, "a", diff(got, plain))
            gpu.set_label_table(None)
            assert diff(gpu.render_labelled(case.p), plain) == 0, (case.what, "a, no table")
            gpu.set_label_table(hidden)
            assert not gpu.render_labelled(case.p).any(), (case.what, "b")
            compared += int(plain[..., 3].astype(bool).sum())
            if case.q is None:
                gpu.set_labels(np.full(case.vox.shape, 7, np.uint8))
                gpu.set_label_table(half)
                faded = gpu.render_labelled(case.p)
                gpu.set_transfer_fn(np.asarray(case.tf, np.float32) * np.float32(0.5), case.esl)
                want = gpu.render_volume(case.p)
                assert diff(faded, want) == 0, (case.what, "c", diff(faded, want))
                halved += int(want[..., 3].astype(bool).sum())
    assert compared > 24 * 200 and halved > 8 * 200, (compared, halved)


def test_every_path_agrees(vr, gpu, golden, oracle, volumes):
    """Placement and addressing only: linear / bricked, forced planes -1 and 0-9, wide addressing 0 / 1 / 2 / 4, every lane order x wave
    shape x two phases, tile scheduling 0 / 1 / 2 — the restatement's bytes, never a run copy or a column window, never a measured order; u8
    (label bricks behind the field's tables, linear labels elsewhere) and u16 (oct bricks), random labels; a lit frame of the default mode
    and a shadowed frame of the full march with the cue"""
    ref = LabelRef.instance()
    entries = table()
    for name, expect in PATH_VOLUMES:
        views = [v for v in lit_views(vr, golden, name) if v[0] in ("view0", "view1", "view6")]
        cases = []
        for k, (label, view) in enumerate(views):
            cases.append(plain_case(vr, golden, oracle, volumes, name, view, 1 + k % 2, False, what=(name, label, "lit"), lighting=PHONG))
            cases.append(plain_case(vr, golden, oracle, volumes, name, view, 1 + k % 2, True, what=(name, label, "cue"), set_clip=CLIPS["both"], clip=CLIPS["both"]))
        vox = cases[0].vox
        labels = random_labels(vox, 1)
        load(gpu, vox, cases[0].tf, cases[0].esl)
        gpu.set_labels(labels)
        gpu.set_label_table(entries)
        seen = set()

        def check_all(what):
            for case in cases:
                set_state(gpu, case)
                case.what = case.what[:3] + (what,)
                check(gpu, ref, case, labels, entries)
                seen.add(gpu.last_launch()["layout"])
        sweep_paths(vr, gpu, check_all)
        assert seen == expect, (name, seen)


def test_bands_crop_and_device_entry_point(vr, gpu, golden, oracle, volumes):
    """Three ranks of interleaved 16-row bands (a view of 70 rows: 5 bands, so two ranks hold a band beyond the view, which is zero) and a
    crop in x equal the matching rows / columns of the whole frame; the device entry point renders the same in one launch, from labels
    given as a device tensor"""
    import torch
    name = "blob_40x24x56"
    ref = LabelRef.instance()
    entries = table()
    case = plain_case(vr, golden, oracle, volumes, name, vr.benchmark_view(120, 70, 5), 1, False, lighting=PHONG)
    labels = structured_labels(case.vox)
    load(gpu, case.vox, case.tf, case.esl)
    gpu.set_labels(torch.from_numpy(np.array(labels)).cuda())
    gpu.set_label_table([vr.binding.make_label_entry(e[:3], e[3], e[4]) for e in entries])
    set_state(gpu, case)
    whole = case.p
    want = check(gpu, ref, case, labels, entries).frame
    assert want[..., 3].astype(bool).sum() > 1000
    for rank in range(3):
        p, per_rank = vr.band_partition(whole.copy(), rank, 3, 16)
        rows = per_rank * 16
        assert p.out_rows == rows == 32
        assert diff(gpu.render_labelled(p), expected_bands(want, rank, 3, 16, rows)) == 0, rank
    crop = whole.copy()
    crop.x0, crop.out_width = 24, 40
    assert diff(gpu.render_labelled(crop), want[:, 24:64]) == 0
    frame = torch.full((70, 120, 4), 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                            # (the fill runs on torch's stream, the frame on the context's)
    gpu.timing_reset()
    before = gpu.labelled_frames()
    gpu.render_labelled_device(whole, frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert gpu.timing().launches == 1 and gpu.labelled_frames() == before + 1 and label_launch(gpu.last_launch())
    assert diff(frame.cpu().numpy(), want) == 0


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
def test_edge_shapes(vr, gpu, oracle, dtype):
    """EDGE_SHAPES of tests/feature_random.py (extents of 1, 2, 8, 9, 33 and 65: brick edges, ragged last bricks, the table pad) from views
    0, 1 and 5 at 48 x 40 (no multiple of the tile) under both clips of its frames, with their esl and thresholds, random labels, the
    shading cycling through the cue, the lighting, the shadow and both"""
    ref = LabelRef.instance()
    entries = table()
    gpu.set_window_buffer(*fr.EDGE_SIZE)
    gpu.set_label_table(entries)
    frames = 0
    for i, shape in enumerate(fr.EDGE_SHAPES):
        s = fr.edge_scene(oracle, vr, shape, dtype)
        labels = random_labels(s.vox, 2)
        gpu.set_transfer_fn(s.tf, s.esl)
        gpu.set_volume(s.vox)
        gpu.set_labels(labels)
        for j, f in enumerate(s.frames):
            case = random_case(s, j, f, (i + j) % 4)
            case.what = (shape, dtype, f.view, f.clip_name) + case.what[3:4]
            set_state(gpu, case)
            check(gpu, ref, case, labels, entries)
            frames += 1
    assert frames == len(fr.EDGE_SHAPES) * len(fr.EDGE_VIEWS) * len(fr.EDGE_CLIPS)


def test_state(vr, gpu, golden, oracle, volumes):
    """Labels replaced and dropped, the table changed between frames, set_volume and generate_volume drop the labels and keep the table, the
    frame counter, every error of step 11, and what labels and a table leave alone: every other frame kind — composite, MIP,
    isosurface, section, depth — keeps its bytes and its counters"""
    import torch
    ref = LabelRef.instance()
    case = plain_case(vr, golden, oracle, volumes, "bucky", vr.benchmark_view(128, 128, 1), 1, False)
    vox, p = case.vox, case.p
    load(gpu, vox, case.tf, case.esl)
    first = gpu.render_volume(p)
    others = (gpu.render_mip(p), gpu.render_iso(p, 100.0), gpu.render_section(p, (0.0, 0.0, 1.0, 0.1)), gpu.render_depth(p, 0.5))
    counters = gpu.lighting_frames(), gpu.preint_frames(), gpu.backdrop_frames(), gpu.section_frames(), gpu.depth_frames()
    L = vr.lib()
    out = np.zeros((p.out_rows, p.out_width, 4), np.uint8)
    dev = torch.zeros((p.out_rows, p.out_width, 4), dtype=torch.uint8, device="cuda")

    def refused(params):
        return [L.vr_hip_render_labelled(gpu._ctx, C.byref(params), out.ctypes.data), L.vr_hip_render_labelled_device(gpu._ctx, C.byref(params), dev.data_ptr(), None)]
    count = gpu.labelled_frames()
    assert refused(p) == [5, 5]                         # VR_ERR_NOT_READY: no labels yet
    a, b = structured_labels(vox), random_labels(vox, 3)
    wrong_dims = np.zeros((vox.shape[0], vox.shape[1], vox.shape[2] + 1), np.uint8)
    with pytest.raises(vr.VrError) as e:
        gpu.set_labels(wrong_dims)
    assert e.value.code == 1 and "dims" in str(e.value) and refused(p) == [5, 5]
    entries = table()
    gpu.set_labels(a)
    gpu.set_label_table(entries)
    check(gpu, ref, case, a, entries)
    gpu.set_labels(b)                                   # replaced: the label bricks are rebuilt
    check(gpu, ref, case, b, entries)
    swapped = entries[::-1].copy()
    gpu.set_label_table(swapped)                        # the table changed between frames
    check(gpu, ref, case, b, swapped)
    gpu.set_label_table(swapped[:3])                    # the rest are identity again
    check(gpu, ref, case, b, swapped[:3])
    assert gpu.labelled_frames() == count + 4
    # errors
    nearest = p.copy()
    nearest.sampling = 0
    assert refused(nearest) == [1, 1]
    with pytest.raises(vr.VrError) as e:
        gpu.render_labelled(nearest)
    assert e.value.code == 1 and "TRILINEAR" in str(e.value)
    gpu.set_preintegration()
    assert refused(p) == [1, 1]
    gpu.clear_preintegration()
    E = vr.VrLabelEntry
    too_many = (E * 257)()
    assert L.vr_hip_set_label_table(gpu._ctx, too_many, 257) == 1 and L.vr_hip_set_label_table(gpu._ctx, None, 1) == 1
    nan, inf = float("nan"), float("inf")
    for member in range(5):
        for value in (nan, inf, -inf, -0.25, 1.5):
            e5 = [0.5, 0.5, 0.5, 0.5, 0.5]
            e5[member] = value
            one = (E * 1)(vr.binding.make_label_entry(e5[:3], e5[3], e5[4]))
            assert L.vr_hip_set_label_table(gpu._ctx, one, 1) == 1, (member, value)
    assert L.vr_hip_render_labelled(gpu._ctx, C.byref(p), None) == 1 and L.vr_hip_render_labelled_device(gpu._ctx, None, dev.data_ptr(), None) == 1
    assert L.vr_hip_labelled_frames(gpu._ctx, None) == 1
    check(gpu, ref, case, b, swapped[:3])               # a refused table leaves the one before in place
    assert gpu.labelled_frames() == count + 5
    # what labels and a table leave alone
    again = (gpu.render_mip(p), gpu.render_iso(p, 100.0), gpu.render_section(p, (0.0, 0.0, 1.0, 0.1)), gpu.render_depth(p, 0.5))
    for x, y in zip(others, again):
        assert np.array_equal(x, y)
    assert np.array_equal(gpu.render_volume(p), first)
    assert (gpu.lighting_frames(), gpu.preint_frames(), gpu.backdrop_frames(), gpu.section_frames(), gpu.depth_frames()) == tuple(n + (i >= 3) for i, n in enumerate(counters))
    # dropped
    gpu.clear_labels()
    assert refused(p) == [5, 5]
    gpu.set_labels(b)
    gpu.set_volume(vox)                                 # a new volume drops the labels; the table stays
    assert refused(p) == [5, 5]
    gpu.set_labels(b)
    check(gpu, ref, case, b, swapped[:3])
    gpu.generate_volume("shell", 32)
    assert refused(p) == [5, 5] and gpu.labelled_frames() == count + 6


@needs_bounds_lib
def test_labelled_frames_under_the_bounds_checked_build():
    """A subset of this file once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every gather address —
    the label's among them — is held against its array: a violation fails the frame (VrError), and the bytes still equal the restatement"""
    run_under_bounds_build(__file__, "edge_shapes or every_path or (frames_equal and random_u16)", 5, timeout=900)


def test_driver_label_flags(golden, tmp_path):
    """volr_bench -labels-octants / -label (HipRenderer::set_labels, set_label_table, set_labelled through the host mirror): Bucky.pvm,
    TRILINEAR, pose (-45,-45,0) at distance 2, 256 x 256 — the frame is the restatement's with the octant labels and the table given on the
    command line; -labels <file> gives the same from a raw file; NEAREST and a device list are refused, and -label needs labels"""
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    st = golden.volume_state("bucky")
    case = next(c for c in golden.cases(True) if c["label"] == "bench256_view1_default")
    p = golden.params(case, 1)
    z, y, x = vox.shape
    zz, yy, xx = np.mgrid[0:z, 0:y, 0:x]
    octants = ((xx >= x // 2) + 2 * (yy >= y // 2) + 4 * (zz >= z // 2)).astype(np.uint8)
    entries = identity_table(8)
    entries[1] = (1.0, 0.0, 0.0, 1.0, 1.0)
    entries[2] = (0.0, 0.0, 0.0, 0.0, 0.0)
    entries[5] = (0.0, 0.5, 1.0, 0.5, 0.75)
    flags = []
    for i in (1, 2, 5):
        flags += ["-label", str(i)] + [repr(float(v)) for v in entries[i]]
    want = LabelRef.instance().render(p, vox, st["tf"], st["esl"], octants, entries).frame
    out, rgb = run_driver(tmp_path, "-labels-octants", *flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Labels:" in out.stdout and np.array_equal(rgb, want[..., :3]), int((rgb != want[..., :3]).any(axis=-1).sum())
    raw = tmp_path / "octants.raw"
    raw.write_bytes(octants.tobytes())
    out, rgb = run_driver(tmp_path, "-labels", str(raw), *flags)
    assert out.returncode == 0 and np.array_equal(rgb, want[..., :3]), out.stdout + out.stderr
    plain, rgb_plain = run_driver(tmp_path)
    assert plain.returncode == 0 and (rgb_plain != rgb).any(axis=-1).sum() > 2000
    for bad in (["-devices", "0,0"], ["-r", "0"], ["-mip"]):
        out, _ = run_driver(tmp_path, *bad, "-labels-octants", size=(128, 128), pose=None, renderer=None if "-r" in bad else "1", output=None)
        assert out.returncode != 0 and "Error: -labels" in out.stdout, (bad, out.stdout)
    out, _ = run_driver(tmp_path, "-label", "1", "1", "0", "0", "1", "1", size=(128, 128), pose=None, output=None)
    assert out.returncode != 0 and "need -labels" in out.stdout, out.stdout
