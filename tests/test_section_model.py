"""CPU tier of the section frames (include/vr_hip.h vr_hip_render_section / vr_hip_render_section_in_volume): section_render of
tests/section_ref.c — the frames and depths the GPU tier expects — is tied to the clipped MIP restatement and to a numpy restatement of
the colouring, the frames of the GPU tier's main test are shown to carry sections (so that test cannot pass by being empty) and to tell
four wrong readings of the contract apart, and the section kernels are held to the registers of their mip_clipped twins.
A reading this restatement and its kernel SHARE is not visible here: tests/test_f64_model.py holds the restatement, and tests/test_gpu_f64_model.py the
kernel, to an independent float64 statement of the contract (tests/f64_model.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clip_helpers import BOTH, IDENTITY, ClipRef
from helpers import axis_view
from light_helpers import lit_views, lit_volumes
from section_helpers import (KX_LT_KC, MEAN_N_PLUS_1, MIN_FROM_0, MODES, SECTION_VOLUMES, THICK_DEPTH_KC, THICK_ON_KC, WINDOWS, SectionRef, half_width_of, planes_of,
                             tier_frames, unit)
from slab_helpers import slab_scene

MISS = 0xffffffff
NEW_SYMBOLS = ("vr_hip_render_section", "vr_hip_render_section_device", "vr_hip_render_section_in_volume", "vr_hip_render_section_in_volume_device",
               "vr_hip_section_frames")


def diff(a, b):
    return int((a != b).any(axis=-1).sum())


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.mark.parametrize("name", SECTION_VOLUMES)
def test_modes_are_tied_on_one_frame(vr, golden, oracle, volumes, name):
    """With the plane facing the view (no ray runs inside it) and a slab that contains the whole cube (h = 4) the narrowing changes no
    segment: the MAX frame coloured by the transfer function is clip_mip_render's under the same clip, byte for byte — under the identity
    clip and under a box with a cutting plane —, its depth is the clipped kx, and MIN <= MEAN <= MAX per pixel, in value and in the grey
    window's bytes.  The POINT frame of the same plane holds exactly one sample per section pixel, depth -1 everywhere else, and equals each
    thick mode evaluated on [kc, kc]: frame, depth bits and value bits."""
    ref, clip_ref = SectionRef.instance(), ClipRef.instance()
    for label, view in lit_views(vr, golden, name)[1::3]:
        plane = unit(tuple(view.direction)) + (0.0,)
        for sampling in (1, 2):
            vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, sampling, True)
            for clip in (IDENTITY, BOTH):
                out, depth, count, vmax = ref.render(p, vox, tf, plane, 4.0, "max", None, clip)
                assert diff(out, clip_ref.mip(p, vox, tf, clip)) == 0, (name, label, sampling, clip)
                hit = (count != MISS) & (count > 0)
                assert hit.sum() > 200 and np.array_equal(hit, count != MISS) and np.array_equal(depth == -1.0, ~hit)
                vmin, vmean = (ref.render(p, vox, tf, plane, 4.0, mode, None, clip)[3] for mode in ("min", "mean"))
                assert (vmin[hit] <= vmean[hit]).all() and (vmean[hit] <= vmax[hit]).all() and (vmin[hit] < vmax[hit]).any()
                grey = [ref.render(p, vox, tf, plane, 4.0, mode, WINDOWS[name], clip)[0] for mode in ("min", "mean", "max")]
                assert (grey[0][hit] <= grey[1][hit]).all() and (grey[1][hit] <= grey[2][hit]).all() and (grey[2][hit][:, 3] == 255).all()
                point, pdepth, pcount, pvalue = ref.render(p, vox, tf, plane, 0.0, "point", None, clip)
                on = pcount == 1
                assert on.sum() > 200 and np.array_equal(on, (pcount != MISS) & (pcount != 0)) and np.array_equal(pdepth == -1.0, ~on)
                assert np.isfinite(pvalue[on]).all()
                for mode in ("max", "min", "mean"):         # POINT is each thick mode evaluated on [kc, kc]
                    thick = ref.render(p, vox, tf, plane, 0.0, mode, None, clip, perturb=THICK_ON_KC)
                    assert diff(thick[0], point) == 0 and np.array_equal(bits(thick[1]), bits(pdepth)) and np.array_equal(bits(thick[3]), bits(pvalue)), mode


def test_window_colouring_and_depth(vr, golden, oracle, volumes):
    """Step 6 restated in numpy on a u8 volume under the window {0, 255} at POINT: inv = 1.0f / (hi - lo) once, g = the product of the
    rounded difference, clamped to [0, 1], the byte (uint8) min(g * 256, 255) three times and alpha 255.  Depth is -1 exactly where the
    pixel is the miss word (a windowed section pixel is opaque), and a POINT depth is kc, the same bits whatever the colouring."""
    ref = SectionRef.instance()
    name = "bucky"
    seen = 0
    for label, view in lit_views(vr, golden, name)[::2]:
        vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1, True)
        for section_label, plane, clip in planes_of(view):
            out, depth, count, value = ref.render(p, vox, tf, plane, 0.0, "point", (0.0, 255.0), clip)
            hit = count == 1
            inv = np.float32(1.0) / (np.float32(255.0) - np.float32(0.0))
            g = np.clip(((value[hit] - np.float32(0.0)).astype(np.float32) * inv).astype(np.float32), np.float32(0.0), np.float32(1.0))
            byte = np.minimum((g * np.float32(256.0)).astype(np.float32).astype(np.int64), 255).astype(np.uint8)
            assert np.array_equal(out[hit][:, 0], byte) and np.array_equal(out[hit][:, 1], byte) and np.array_equal(out[hit][:, 2], byte)
            assert (out[hit][:, 3] == 255).all() and not out[~hit].any()
            assert np.array_equal(depth == -1.0, ~hit) and np.array_equal(out.view(np.uint32)[..., 0] == 0, ~hit)
            by_tf = ref.render(p, vox, tf, plane, 0.0, "point", None, clip)
            assert np.array_equal(bits(by_tf[1]), bits(depth)) and not by_tf[0][~hit].any()
            seen += int(hit.sum())
    assert seen > 20000, seen


def test_a_ray_inside_the_plane_is_a_miss(vr, oracle):
    """An orthogonal view along z and the section x = 0: n . direction is exactly 0 for every ray, an all-miss frame in every mode,
    though every ray crosses the cube"""
    ref = SectionRef.instance()
    rng = np.random.default_rng(3)
    vox = rng.integers(1, 255, size=(24, 24, 24), dtype=np.uint8)
    tf, esl, bd, bs, step = oracle.scene_for(vox)
    p = vr.VrParams()
    p.view = axis_view(vr, (24, 24, 24), 2, 1, cells_per_pixel=0.5, margin=0)
    p.ray_step, p.ray_threshold, p.light_kd, p.esl, p.esl_block_dims = float(step), 1.0, 0.0, 0, 1
    p.sampling = 1
    p = vr.whole_frame(p)
    assert sorted(abs(c) for c in p.view.direction) == [0.0, 0.0, 1.0]
    for mode in MODES:
        out, depth, count, _ = ref.render(p, vox, tf, (1.0, 0.0, 0.0, 0.0), 0.0 if mode == "point" else 0.3, mode, (0.0, 255.0))
        assert not out.any() and (depth == -1.0).all() and (count == 0).all(), mode
    out, depth, count, _ = ref.render(p, vox, tf, (0.0, 0.0, 1.0, 0.0), 0.0, "point", (0.0, 255.0))
    assert (count == 1).all() and (out[..., 3] == 255).all()


@pytest.mark.parametrize("name", SECTION_VOLUMES)
def test_the_main_tests_frames_carry_sections_and_tell_wrong_readings_apart(vr, golden, oracle, volumes, name):
    """The list tier_frames gives tests/test_gpu_section.py, on the restatement alone.
    Conditions: at least a fifth of the rays that hit the (clipped) cube carry a section in every frame; in the thick frames at least half
    of the section pixels hold two or more samples; under the grey window the MAX, MIN and MEAN frames of a (view, section) differ
    pairwise in at least a fifth of the section pixels.
    Sensitivity, per wrong reading the frames it can show in: `kx < kc` in the POINT frames of the cut sections (the clip plane on the
    section: kx == kc bit for bit) — all of them change; the mean over n + 1 in the MEAN frames — all; the depth of a thick pixel = kc in
    the thick frames of the other five sections (on a cut section kx IS kc) — all; MIN started at 0 in the MIN frames — all: the plateau's
    sections are tilted and narrower than its block, so that every MIN frame holds rays whose slab lies wholly inside the block (minimum
    200) beside the rays that straddle its faces, and Bucky's MIN frames take the window from 0, under which every minimum of 1 or more
    shows (section_helpers.planes_of, ALWAYS_WINDOWED).  The counts are in DESIGN.md section 4.12."""
    ref = SectionRef.instance()
    applies = {KX_LT_KC: lambda what: what[4] == "point" and what[3] == "cut", MEAN_N_PLUS_1: lambda what: what[4] == "mean",
               MIN_FROM_0: lambda what: what[4] == "min", THICK_DEPTH_KC: lambda what: what[4] != "point" and what[3] != "cut"}
    changed, applied, frames, grey = dict.fromkeys(applies, 0), dict.fromkeys(applies, 0), 0, {}
    for sampling in (1, 2):
        for what, vox, p, tf, plane, h, mode, window, clip in tier_frames(vr, golden, oracle, volumes, name, sampling):
            out, depth, count, value = ref.render(p, vox, tf, plane, h, mode, window, clip)
            frames += 1
            rays = count != MISS
            section = rays & (count > 0)
            assert rays.sum() >= 100 and 5 * section.sum() >= rays.sum(), (what, int(rays.sum()), int(section.sum()))
            if mode != "point":
                assert 2 * (count[section] >= 2).sum() >= section.sum(), (what, int(section.sum()))
                if window is not None:
                    grey[what[:4] + (mode,)] = out
                    if mode == "mean":
                        a, b = grey[what[:4] + ("max",)], grey[what[:4] + ("min",)]
                        for x, y in ((a, b), (a, out), (b, out)):
                            assert 5 * ((x != y).any(axis=-1) & section).sum() >= section.sum(), what
            else:
                assert (count[section] == 1).all()
            for perturb, fits in applies.items():
                if fits(what):
                    wrong = ref.render(p, vox, tf, plane, h, mode, window, clip, perturb=perturb)
                    applied[perturb] += 1
                    changed[perturb] += int(diff(wrong[0], out) > 0 or not np.array_equal(bits(wrong[1]), bits(depth)))
    print(f"{name}: {frames} frames; changed / applies: kx < kc {changed[KX_LT_KC]}/{applied[KX_LT_KC]}, mean over n + 1 {changed[MEAN_N_PLUS_1]}/{applied[MEAN_N_PLUS_1]}, "
          f"MIN from 0 {changed[MIN_FROM_0]}/{applied[MIN_FROM_0]}, thick depth = kc {changed[THICK_DEPTH_KC]}/{applied[THICK_DEPTH_KC]}")
    assert frames == 432 and applied == {KX_LT_KC: 18, MEAN_N_PLUS_1: 108, MIN_FROM_0: 108, THICK_DEPTH_KC: 270}
    assert changed == applied, (changed, applied)


def test_in_volume_is_the_section_then_the_backdrop(vr, golden, oracle, volumes):
    """section_in_volume_render is section_render followed by backdrop_render in place: its section frame and depth are section_render's,
    and the frame differs from the section frame (volume in front of it) and from the plain composite (the section behind it)"""
    from backdrop_helpers import BackdropRef
    ref, backdrop = SectionRef.instance(), BackdropRef.instance()
    name = "bucky"
    label, view = lit_views(vr, golden, name)[1]
    vox, p, tf, esl = slab_scene(vr, golden, oracle, volumes, name, view, 1, False)
    plane = planes_of(view)[1][1]
    for mode, window in (("point", WINDOWS[name]), ("mean", None)):
        h = 0.0 if mode == "point" else half_width_of(p, name)
        out, depth, section = ref.in_volume(p, vox, tf, esl, plane, h, mode, window)
        alone = ref.render(p, vox, tf, plane, h, mode, window)
        assert diff(section, alone[0]) == 0 and np.array_equal(bits(depth), bits(alone[1]))
        assert diff(out, backdrop.render(p, vox, tf, esl, alone[0], alone[1])) == 0
        assert diff(out, section) > 500 and diff(out, backdrop.render(p, vox, tf, esl)) > 500


def _kernels(text, pattern):
    out = {}
    for m in re.finditer(r"Function Name: (\S*?" + pattern + r"\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        out[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    return out


ROWS = r"ILi(\d)ELi(\d)ELi(\d)ELi(\d)E"


def test_section_kernels_keep_eight_waves(vr):
    """The sixth log, resource_usage_section.log: 24 names, each once and in no other log — section_kernel over the 24 rows of the
    isosurface.  No scratch, no SGPR or VGPR spilled.  Every mip_clipped twin of the same (SAMPLING, BPV, ADDR, LAYOUT) in
    resource_usage.log keeps <= 80 SGPRs and <= 64 VGPRs (8 waves per SIMD), so every section kernel must too: no row takes the
    allowance for minimum, sum and count.  The other five logs keep their 269 / 36 / 24 / 48 / 96 names."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    logs = [os.path.join(csrc, n) for n in ("resource_usage.log", "resource_usage_shadow.log", "resource_usage_light.log", "resource_usage_slab.log",
                                            "resource_usage_backdrop.log", "resource_usage_section.log")]
    if not all(os.path.exists(p) for p in logs):
        subprocess.check_call(["make", "-B", "-C", csrc])
    texts = [open(p).read() for p in logs]
    names = [re.findall(r"Function Name: (\S+)", t) for t in texts]
    assert [len(n) for n in names] == [269, 36, 24, 48, 96, 24], [len(n) for n in names]
    assert len(set(sum(names, []))) == 269 + 36 + 24 + 48 + 96 + 24
    assert all("section_kernel" in n for n in names[5]) and not [n for n in sum(names[:5], []) if "section" in n]
    assert not [n for n in names[5] if "raymarch_kernel" in n or "colmarch_" in n]
    key = lambda name: tuple(int(g) for g in re.search(ROWS, name).groups())      # noqa: E731
    mine = {key(n): v for n, v in _kernels(texts[5], r"\d+section_kernel" + ROWS.replace("(", "(?:")).items()}
    twins = {key(n): v for n, v in _kernels(texts[0], r"\d+mip_clipped" + ROWS.replace("(", "(?:")).items()}
    iso_rows = {key(n) for n in names[0] if re.search(r"\d+iso_clipped" + ROWS, n)}
    assert len(mine) == 24 and set(mine) == iso_rows and set(mine) <= set(twins)
    for row, (sgprs, vgprs, scratch, occupancy, sspill, vspill) in mine.items():
        t_sgprs, t_vgprs = twins[row][:2]
        assert scratch == 0 and sspill == 0 and vspill == 0, (row, scratch, sspill, vspill)
        assert t_sgprs <= 80 and t_vgprs <= 64, (row, twins[row])
        assert sgprs <= 80 and vgprs <= 64 and occupancy == 8, (row, sgprs, vgprs, occupancy)


def test_binding_and_header(vr):
    """vr_section is 32 bytes with plane, half_width, mode, window at offsets 0 / 16 / 20 / 24; vr_params keeps its 132 bytes, VrLaunchInfo its
    13 members and 52 bytes; the five entry points are declared in include/vr_hip.h, exported and resolved by the binding; without a
    context they return VR_ERR_INVALID; the renderer has the methods, the device list does not."""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    L = vr.lib()
    raw = C.CDLL(vr.library_path())
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert hasattr(L, name) and hasattr(raw, name), name
    assert re.search(r"typedef struct vr_section \{\s*float\s+plane\[4\];\s*float\s+half_width;\s*uint32_t\s+mode;\s*float\s+window\[2\];\s*\} vr_section;", text)
    assert re.search(r"VR_SECTION_POINT = 0, VR_SECTION_MAX = 1, VR_SECTION_MIN = 2, VR_SECTION_MEAN = 3", text)
    S = vr.VrSection
    assert C.sizeof(S) == 32 and (S.plane.offset, S.half_width.offset, S.mode.offset, S.window.offset) == (0, 16, 20, 24)
    assert C.sizeof(vr.VrParams) == 132 and len(vr.VrLaunchInfo._fields_) == 13 and C.sizeof(vr.VrLaunchInfo) == 52
    p, sec, count = vr.VrParams(), vr.VrSection(), C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    assert L.vr_hip_render_section(None, C.byref(p), C.byref(sec), buf, None) == 1
    assert L.vr_hip_render_section_device(None, C.byref(p), C.byref(sec), buf, None, None) == 1
    assert L.vr_hip_render_section_in_volume(None, C.byref(p), C.byref(sec), buf, None) == 1
    assert L.vr_hip_render_section_in_volume_device(None, C.byref(p), C.byref(sec), buf, None, None) == 1
    assert L.vr_hip_section_frames(None, C.byref(count)) == 1
    for method in ("render_section", "render_section_device", "render_section_in_volume", "render_section_in_volume_device", "section_frames"):
        assert callable(getattr(vr.HipRenderer, method)), method
    assert not hasattr(vr.MultiRenderer, "render_section")        # single device: the device list stays without it
