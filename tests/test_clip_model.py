"""CPU tier of the clip region (include/vr_hip.h vr_hip_set_clip): the clip_* entry points of tests/feature_ref.c — the frames and depths the GPU
tier expects — tied to the oracle's vro_render (clip_render_ray is a text of its own) and to the unclipped mip_render and iso_render, held against the geometry of the
region itself, and shown to be neither empty nor unclipped on what the GPU tier renders; the register figures of the built *_clipped
kernels; the layout of VrClip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clip_helpers import BOTH, BOX, CLIPS, IDENTITY, NOTHING, PLANE, ClipRef, clip_floats, composite_params, parallel_plane
from iso_helpers import PAIRS, IsoRef, all_volumes, depth_bits, frame_params, views_for
from mip_helpers import MipRef, ramp_tf

SMALL_CASES = (32, 34, 36, 38, 40, 45)        # the golden cases tests/test_mip_model.py uses: no ESL, at most 120 x 96 pixels
COMPOSITE_VOLUMES = ("bucky", "blob_40x24x56", "random_u16")             # what tests/test_gpu_clip.py composites
PROJECTION_VOLUMES = ("late_max", "corner", "blob_40x24x56", "random_u16")      # ... and projects (MIP, isosurface)
LEVELS = {name: [level for n, level in PAIRS if n == name] for name in PROJECTION_VOLUMES}
REFINE = 4


def test_identity_clip_is_the_unclipped_oracle_on_every_golden_case(golden, oracle):
    """The box [-1,1]^3 without a plane changes no bit of [kx, ky]: clip_render is then render_ray of oracle/vr_oracle.c, NEAREST and
    TRILINEAR, default mode and full march, every golden case that carries a frame"""
    ref = ClipRef.instance()
    checked = 0
    for case in golden.cases(True):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        for sampling in (0, 1, 2):
            p = golden.params(case, sampling)
            want = oracle.render(p, vox, st["tf"], st["esl"])
            assert np.array_equal(ref.composite(p, vox, st["tf"], st["esl"], IDENTITY), want), (case["label"], sampling)
            checked += int((want[..., 3] != 0).sum())
    assert checked > 100000, checked


def test_identity_clip_is_the_pinned_mip_and_iso_restatement(golden):
    """... and clip_mip_render / clip_iso_render are mip_render / iso_render, byte for byte and depth bit for depth bit.  Each pair wraps one
    frame function of tests/feature_ref.c, with the clip and without: the tie compares that text with itself under the identity clip, and
    tests/test_restatement_pins.py pins it to the separate texts (mip_ref.c, iso_ref.c, clip_ref.c) it replaced"""
    ref, tf = ClipRef.instance(), ramp_tf()
    hits = 0
    for cid in SMALL_CASES:
        case = next(c for c in golden.cases() if c["id"] == cid)
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        for sampling in (0, 1, 2):
            p = golden.params(case, sampling)
            p.esl, p.ray_threshold = 0, 1.0
            assert np.array_equal(ref.mip(p, vox, tf, IDENTITY), MipRef.instance().render(p, vox, tf)[0]), (cid, sampling)
            if sampling == 0:
                continue
            for level in (30.5, 100.0, 200.0):
                for refine in (0, REFINE):
                    want, want_depth, counters = IsoRef.instance().render(p, vox, tf, level, refine)
                    got, depth, _ = ref.iso(p, vox, tf, level, refine, IDENTITY)
                    assert np.array_equal(got, want) and np.array_equal(depth_bits(depth), depth_bits(want_depth)), (cid, sampling, level, refine)
                    hits += counters["hits"]
    assert hits > 10000, hits


def _gpu_tier_frames(vr, golden, oracle, clip):
    """(volume, what, clipped frame, unclipped frame) of everything tests/test_gpu_clip.py compares per (volume, view set, clip), one
    sampling each: the composite in default mode, the MIP, the isosurface"""
    ref, tf, volumes = ClipRef.instance(), ramp_tf(), all_volumes(golden)
    for name in COMPOSITE_VOLUMES:
        for label, view in views_for(vr, golden, name):
            p, ctf, esl = composite_params(vr, golden, oracle, name, volumes[name], view, 1, False)
            yield name, "composite", ref.composite(p, volumes[name], ctf, esl, clip), ref.composite(p, volumes[name], ctf, esl, IDENTITY)
    for name in PROJECTION_VOLUMES:
        for label, view in views_for(vr, golden, name):
            p = frame_params(vr, oracle, volumes[name], view, 1, 0)
            yield name, "mip", ref.mip(p, volumes[name], tf, clip), ref.mip(p, volumes[name], tf, IDENTITY)
            for level in LEVELS[name]:
                yield name, f"iso@{level}", ref.iso(p, volumes[name], tf, level, REFINE, clip)[0], ref.iso(p, volumes[name], tf, level, REFINE, IDENTITY)[0]


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
def test_gpu_tier_frames_are_neither_empty_nor_unclipped(vr, golden, oracle, clip_name):
    """The cap: for every (volume, view set, clip) of the GPU tier — per volume and clip, the composite frames of
    test_composite_equals_the_restatement and the MIP + isosurface frames of test_mip_and_isosurface_equal_the_restatement, each summed over
    the nine views — at least 5 % of the pixels are non-zero in the clipped reference and at least 5 % differ from the unclipped one: the
    GPU tier cannot pass on empty or on unclipped frames.  (Per projection the figures are printed, not held: `corner` is one bright voxel,
    its isosurface a handful of pixels with or without a clip, and its level 200 is never reached.)"""
    totals, detail = {}, {}
    for name, what, clipped, plain in _gpu_tier_frames(vr, golden, oracle, CLIPS[clip_name]):
        for table, key in ((totals, (name, "composite" if what == "composite" else "projections")), (detail, (name, what))):
            t = table.setdefault(key, [0, 0, 0])
            t[0] += int(clipped.any(axis=-1).sum())
            t[1] += int((clipped != plain).any(axis=-1).sum())
            t[2] += clipped.shape[0] * clipped.shape[1]
    for key, (nonzero, differ, pixels) in sorted(detail.items()):
        print(f"{clip_name} {key}: {100 * nonzero / pixels:.1f} % non-zero, {100 * differ / pixels:.1f} % differ from the unclipped frame")
    assert len(totals) == 3 + 4
    for key, (nonzero, differ, pixels) in sorted(totals.items()):
        assert nonzero >= 0.05 * pixels and differ >= 0.05 * pixels, (clip_name, key, nonzero, differ, pixels)


@pytest.mark.parametrize("clip_name", sorted(CLIPS))
def test_surface_points_lie_inside_the_region(vr, golden, oracle, clip_name):
    """Every isosurface depth d != -1 gives a point origin + dir * d of the pixel's own ray that lies inside the box and on the kept side of
    the plane to within 1e-4 model units: three orders above the fp32 rounding of the point, 300 times below a voxel of the 64^3 volumes"""
    ref, tf, volumes = ClipRef.instance(), ramp_tf(), all_volumes(golden)
    cf = clip_floats(CLIPS[clip_name]).astype(np.float64)
    checked = 0
    for name in PROJECTION_VOLUMES:
        for label, view in views_for(vr, golden, name):
            for sampling in (1, 2):
                p = frame_params(vr, oracle, volumes[name], view, sampling, 0)
                for level in LEVELS[name]:
                    _, depth, rays = ref.iso(p, volumes[name], tf, level, REFINE, CLIPS[clip_name])
                    hit = depth != -1
                    pos = rays[hit][:, :3].astype(np.float64) + rays[hit][:, 3:].astype(np.float64) * depth[hit][:, None].astype(np.float64)
                    assert (pos >= cf[0:3] - 1e-4).all() and (pos <= cf[3:6] + 1e-4).all(), (name, label, sampling, level)
                    assert (pos @ cf[6:9] + cf[9] >= -1e-4).all(), (name, label, sampling, level)
                    checked += int(hit.sum())
    assert checked > 20000, checked


def test_nothing_is_kept_behind_a_plane_that_misses_the_cube(vr, golden, oracle):
    ref, tf, volumes = ClipRef.instance(), ramp_tf(), all_volumes(golden)
    vox = volumes["blob_40x24x56"]
    for label, view in views_for(vr, golden, "blob_40x24x56"):
        p, ctf, esl = composite_params(vr, golden, oracle, "blob_40x24x56", vox, view, 1, False)
        assert not ref.composite(p, vox, ctf, esl, NOTHING).any(), label
        q = frame_params(vr, oracle, vox, view, 1, 0)
        assert not ref.mip(q, vox, tf, NOTHING).any(), label
        frame, depth, _ = ref.iso(q, vox, tf, 100.0, REFINE, NOTHING)
        assert not frame.any() and (depth == -1).all(), label


def test_a_plane_along_the_view_keeps_whole_rays_or_none(vr, golden, oracle):
    """PARALLEL: the normal is the screen-right axis of benchmark view 0, n . direction is exactly 0 on that orthogonal view, so every ray is
    kept unchanged or missed as a whole: the kept pixels equal the unclipped ones, the others are empty, and between 30 % and 70 % of the
    unclipped non-zero pixels are kept (the plane passes through the centre)"""
    ref, tf, volumes = ClipRef.instance(), ramp_tf(), all_volumes(golden)
    for name in ("bucky", "late_max"):
        vox = volumes[name]
        view = vr.benchmark_view(80, 80, 0)
        clip = parallel_plane(view)
        n, d = np.array(clip[2][:3], np.float32), np.array(list(view.direction), np.float32)
        assert np.float32(np.float32(n[0] * d[0]) + np.float32(n[1] * d[1])) + np.float32(n[2] * d[2]) == 0 and float(n @ n) > 0.99
        p = frame_params(vr, oracle, vox, view, 1, 0)
        plain, kept = ref.mip(p, vox, tf, IDENTITY), ref.mip(p, vox, tf, clip)
        visible, still = plain.any(axis=-1), kept.any(axis=-1)
        assert np.array_equal(kept[still], plain[still]) and not (still & ~visible).any()
        assert 0.3 * visible.sum() <= still.sum() <= 0.7 * visible.sum(), (name, int(still.sum()), int(visible.sum()))
        columns = still.any(axis=0)
        assert not (columns[:39].any() and columns[41:].any()), "the kept rays lie on one side of the screen's centre column"


def test_clipped_kernels_keep_their_registers(vr):
    """Every raymarch_clipped / mip_clipped / iso_clipped instantiation of the build (its resource log): no scratch, no SGPR or VGPR
    spilled, at most 64 VGPRs and at most 96 SGPRs (DESIGN.md section 4.6 has the table); the clipped composite exists for the linear
    array, the quad, voxel and oct bricks over all addressing paths and for no run copy; the MIP / isosurface tables mirror the unclipped ones."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    log = os.path.join(csrc, "resource_usage.log")
    if not os.path.exists(log):
        subprocess.check_call(["make", "-B", "-C", csrc])
    text = open(log).read()
    found = {"raymarch": set(), "mip": set(), "iso": set()}
    twins = {"raymarch": set(), "mip": set(), "iso": set()}
    for m in re.finditer(r"Function Name: (\S*?(raymarch|mip|iso)_(clipped|kernel)ILi(\d)ELi(\d)ELi(\d)ELi(\d)E\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?"
                         r"ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        key = tuple(int(g) for g in m.groups()[3:7])
        if m.group(3) == "kernel":
            twins[m.group(2)].add(key)
            continue
        sgprs, vgprs, scratch, sspill, vspill = (int(g) for g in m.groups()[7:])
        found[m.group(2)].add(key)
        assert scratch == 0 and sspill == 0 and vspill == 0, (m.group(1), scratch, sspill, vspill)
        assert vgprs <= 64 and sgprs <= 96, (m.group(1), sgprs, vgprs)
    assert found["mip"] == twins["mip"] and len(found["mip"]) == 36
    assert found["iso"] == twins["iso"] and len(found["iso"]) == 24
    assert found["raymarch"] == {k for k in twins["raymarch"] if k[3] in (0, 1, 4, 5)} and len(found["raymarch"]) == 36, sorted(found["raymarch"])


def test_struct_layout_matches_header(vr):
    """VrClip against vr_clip of include/vr_hip.h: ten floats, box_min, box_max, plane, in the header's order"""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vr_clip \{(.*?)\} vr_clip;", text, flags=re.S).group(1)
    members = re.findall(r"(\w+)\[(\d)\]", body)
    assert members == [("box_min", "3"), ("box_max", "3"), ("plane", "4")] and set(re.findall(r"\b(float|double|int|uint\w+)\b", body)) == {"float"}
    assert C.sizeof(vr.VrClip) == 40
    assert (vr.VrClip.box_min.offset, vr.VrClip.box_max.offset, vr.VrClip.plane.offset) == (0, 12, 24)
    assert [n for n, _ in vr.VrClip._fields_] == [n for n, _ in members]
    assert C.sizeof(vr.VrParams) == 132           # the clip is context state: vr_params keeps its size
