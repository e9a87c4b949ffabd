"""CPU tier of the depth frames (include/vr_hip.h vr_hip_render_depth / vr_hip_pick): depth_render of tests/depth_ref.c — the depths, values and
alphas the GPU tier expects — is tied to the composite restatements through the alpha byte, its three modes are held to the relations
the contract implies, the frames of the GPU tier's main test are shown to carry surfaces and rays without one (so that test cannot pass by
being empty) and to tell four wrong readings of the contract apart, and the depth kernels are held to 8 waves per SIMD.
A reading this restatement and its kernel SHARE is not visible here: tests/test_f64_model.py holds the restatement, and tests/test_gpu_f64_model.py the
kernel, to an independent float64 statement of the contract (tests/f64_model.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clip_helpers import ClipRef
from depth_helpers import (ACC_BEFORE, DEPTH_VOLUMES, LIGHTING, MEAN_BY_ALPHA, MODE_NUMBER, MODES, OPACITIES, PEAK_LAST, TERMINATOR_LOST, DepthRef, alpha_byte,
                           tier_frames)
from light_helpers import LightRef, lit_volumes
from shadow_helpers import LIGHTS, ShadowRef
from slab_helpers import POINT, SlabRef

NEW_SYMBOLS = ("vr_hip_render_depth", "vr_hip_render_depth_device", "vr_hip_pick", "vr_hip_depth_frames")
TINY = 1e-45                                            # the smallest positive float32: FIRST at it is the first sample that composites anything
ABOVE_THRESHOLD = 0.97                                  # above the 0.95 of the default mode's frames


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def volumes(golden):
    return lit_volumes(golden)


@pytest.fixture(scope="module", autouse=True)
def the_restatement_speaks_of_the_declared_contract(vr):
    """the mode numbers depth_render takes are those of vr_depth_mode as the binding has them"""
    assert MODE_NUMBER == vr.binding.DEPTH_MODES and (vr.binding.DEPTH_FIRST, vr.binding.DEPTH_PEAK, vr.binding.DEPTH_MEAN) == (0, 1, 2)


@pytest.mark.parametrize("name", DEPTH_VOLUMES)
def test_alpha_is_the_composites_alpha_byte(vr, golden, oracle, volumes, name):
    """Consequence 6 on every frame of the list: map_float_int(alpha, 256) is the alpha byte of the composite frame of the same params under
    the same clip and classification — slab_render (point and slab), and for the point-classified frames clip_render (the independent
    composite text); the same bytes again lit by PHONG and scaled by a light grid at strength 0.6 (light_render, slab_render,
    shadow_render): alpha is untouched by both.  The alpha is the same bits in the three modes and at both opacities."""
    ref, slab, clips, light, shadow = DepthRef.instance(), SlabRef.instance(), ClipRef.instance(), LightRef.instance(), ShadowRef.instance()
    lo, hi = OPACITIES[name]
    q = None
    frames = nonzero = 0
    for sampling in (1, 2):
        for what, vox, p, tf, esl, clip, cmode in tier_frames(vr, golden, oracle, volumes, name, sampling):
            if q is None:
                q = shadow.build(LIGHTS["top"], 9, p.ray_step, vox, tf)
            d = ref.render(p, vox, tf, esl, lo, "mean", cmode, clip)
            for mode, opacity in (("first", lo), ("first", hi), ("peak", lo), ("mean", hi)):
                assert np.array_equal(bits(ref.render(p, vox, tf, esl, opacity, mode, cmode, clip).alpha), bits(d.alpha)), (what, mode, opacity)
            byte = alpha_byte(d.alpha)
            assert ((d.alpha >= 0.0) & (d.alpha <= 1.0)).all() and not byte[~d.segment].any(), what
            composites = [slab.render(p, vox, tf, esl, cmode, clip), slab.render(p, vox, tf, esl, cmode, clip, LIGHTING, q, 0.6)]
            if cmode == POINT:
                composites += [clips.composite(p, vox, tf, esl, clip), light.render(p, vox, tf, esl, LIGHTING, q, 0.6, clip), shadow.render(p, vox, tf, esl, q, 0.6, clip)]
            for i, frame in enumerate(composites):
                assert np.array_equal(frame[..., 3], byte), (what, i, int((frame[..., 3] != byte).sum()))
            frames, nonzero = frames + 1, nonzero + int((byte != 0).sum())
    assert frames == 36 and nonzero > 36 * 300, (frames, nonzero)


@pytest.mark.parametrize("name", DEPTH_VOLUMES)
def test_mode_relations(vr, golden, oracle, volumes, name):
    """On every frame of the list.  FIRST: the surfaces shrink and their depth does not decrease as the opacity grows (TINY, the volume's
    two, and ABOVE_THRESHOLD on the frames that terminate early); every surface has depth >= 0 and a finite value, every other pixel -1 / -1.
    PEAK and MEAN have a surface exactly where FIRST at TINY has one — where anything was composited — and their depth lies between that
    depth and the last sample's k: PEAK exactly (it is a sample's k), MEAN within the rounding of its sums — sk and sg are sums of n
    non-negative terms rounded n times each, the quotient once: (n + 2) * 2^-23 relative.  The value of PEAK is the value FIRST or any
    mode could record: between the frame's extremes of the raw voxel range.
    With an opacity above ray_threshold FIRST has a surface only where the terminating sample crossed it: acc > threshold is the only way
    past the opacity, so the surface is the last sample, the ray terminated there, and its alpha is at least the opacity."""
    ref = DepthRef.instance()
    lo, hi = OPACITIES[name]
    top = 255.0 if volumes[name].dtype == np.uint8 else 65535.0
    late = 0
    for sampling in (1, 2):
        for what, vox, p, tf, esl, clip, cmode in tier_frames(vr, golden, oracle, volumes, name, sampling):
            ladder = [TINY, lo, hi] + ([ABOVE_THRESHOLD] if p.ray_threshold < ABOVE_THRESHOLD else [])
            first = [ref.render(p, vox, tf, esl, o, "first", cmode, clip) for o in ladder]
            for shallow, deep in zip(first, first[1:]):
                assert not (deep.surface & ~shallow.surface).any(), what
                assert (deep.depth[deep.surface] >= shallow.depth[deep.surface]).all(), what
            for d in first + [ref.render(p, vox, tf, esl, lo, m, cmode, clip) for m in ("peak", "mean")]:
                assert (d.depth[d.surface] >= 0.0).all() and np.isfinite(d.value[d.surface]).all() and (d.value[d.surface] >= 0.0).all() and (d.value[d.surface] <= top).all(), what
                assert (d.depth[~d.surface] == -1.0).all() and (d.value[~d.surface] == -1.0).all() and not d.surface[~d.segment].any(), what
                assert (d.alpha[~d.surface & (d.count == 0)] == 0.0).all(), what
            any_sample = first[0]
            on = any_sample.surface
            assert np.array_equal(on, any_sample.alpha > 0.0), what
            peak, mean = (ref.render(p, vox, tf, esl, lo, m, cmode, clip) for m in ("peak", "mean"))
            assert np.array_equal(peak.surface, on) and np.array_equal(mean.surface, on), what
            assert (peak.depth[on] >= any_sample.depth[on]).all() and (peak.depth[on] <= peak.last[on]).all(), what
            slack = (mean.count[on].astype(np.float64) + 2.0) * 2.0 ** -23 * mean.last[on].astype(np.float64)
            assert (mean.depth[on] >= any_sample.depth[on] - slack).all() and (mean.depth[on] <= mean.last[on] + slack).all(), what
            if p.ray_threshold < ABOVE_THRESHOLD:
                d = first[-1]
                assert not (d.surface & ~d.terminated).any() and np.array_equal(bits(d.depth[d.surface]), bits(d.last[d.surface])), what
                assert (d.alpha[d.surface] >= np.float32(ABOVE_THRESHOLD)).all() and (d.alpha[d.terminated] > np.float32(p.ray_threshold)).all(), what
                late += int(d.surface.sum())
    assert late > 100, late


@pytest.mark.parametrize("name", DEPTH_VOLUMES)
def test_the_main_tests_frames_carry_surfaces_and_tell_wrong_readings_apart(vr, golden, oracle, volumes, name):
    """The list tier_frames gives tests/test_gpu_depth.py, on the restatement alone, at the two opacities of depth_helpers.OPACITIES.
    Conditions, over the volume's list, per opacity and in every mode: at least a tenth of the rays that hit the cube have a surface; at
    least one in a hundred has none; FIRST and PEAK depths differ on at least one in twenty of the pixels that are a surface in both;
    wide slabs occur under pre-integration.  The shares are printed, and written down in depth_helpers.py.
    Sensitivity, per wrong reading over the frames it can show in: FIRST testing acc before the update (FIRST frames); the terminating
    sample not recorded (every mode, the frames that terminate early); MEAN divided by the final alpha (MEAN frames); PEAK taking the last
    of equal peaks (PEAK frames: a sample with g = 0 then wins on a ray that composites nothing).  Each changes depth bits in the list."""
    ref = DepthRef.instance()
    applies = {ACC_BEFORE: ("first",), TERMINATOR_LOST: MODES, MEAN_BY_ALPHA: ("mean",), PEAK_LAST: ("peak",)}
    changed = dict.fromkeys(applies, 0)
    for opacity in OPACITIES[name]:
        rays, surfaces, both, differ, wide, frames = dict.fromkeys(MODES, 0), dict.fromkeys(MODES, 0), 0, 0, 0, 0
        for sampling in (1, 2):
            for what, vox, p, tf, esl, clip, cmode in tier_frames(vr, golden, oracle, volumes, name, sampling):
                frames += 1
                got = {m: ref.render(p, vox, tf, esl, opacity, m, cmode, clip) for m in MODES}
                for m in MODES:
                    rays[m] += int(got[m].rays.sum())
                    surfaces[m] += int(got[m].surface.sum())
                shared = got["first"].surface & got["peak"].surface
                both, differ = both + int(shared.sum()), differ + int((got["first"].depth[shared] != got["peak"].depth[shared]).sum())
                wide += got["first"].wide if cmode != POINT else 0
                assert got["first"].wide == 0 or cmode != POINT
                for perturb, modes in applies.items():
                    if perturb == TERMINATOR_LOST and not p.esl:
                        continue
                    for m in modes:
                        wrong = ref.render(p, vox, tf, esl, opacity, m, cmode, clip, perturb=perturb)
                        changed[perturb] += int((bits(wrong.depth) != bits(got[m].depth)).sum())
        print(f"{name} opacity {opacity}: {frames} frames; surface / rays " + ", ".join(f"{m} {surfaces[m] / rays[m]:.3f}" for m in MODES) +
              f"; FIRST != PEAK {differ / both:.3f}; wide-slab samples {wide}")
        assert frames == 36
        for m in MODES:
            assert 10 * surfaces[m] >= rays[m] and 100 * (rays[m] - surfaces[m]) >= rays[m], (name, opacity, m, surfaces[m], rays[m])
        assert 20 * differ >= both and wide > 0, (name, opacity, differ, both, wide)
    print(f"{name}: depth bits changed by the wrong readings: {changed}")
    assert all(n > 0 for n in changed.values()), changed


def _kernels(text, pattern):
    out = {}
    for m in re.finditer(r"Function Name: (\S*?" + pattern + r"\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        out[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    return out


ROWS = r"ILi(\d)ELi(\d)ELi(\d)ELi(\d)E"


def test_depth_kernels_keep_eight_waves(vr):
    """The seventh log, resource_usage_depth.log: its names appear once each and in no other log — depth_kernel over the 24 rows of the
    isosurface, and the pick's finishing kernel.  No scratch, no SGPR or VGPR spilled, <= 80 SGPRs and <= 64 VGPRs, 8 waves per SIMD on
    every row, as the mip_clipped twin of the same (SAMPLING, BPV, ADDR, LAYOUT) keeps them.  The six older logs keep their 269 / 36 / 24 /
    48 / 96 / 24 names."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    logs = [os.path.join(csrc, n) for n in ("resource_usage.log", "resource_usage_shadow.log", "resource_usage_light.log", "resource_usage_slab.log",
                                            "resource_usage_backdrop.log", "resource_usage_section.log", "resource_usage_depth.log")]
    if not all(os.path.exists(p) for p in logs):
        subprocess.check_call(["make", "-B", "-C", csrc])
    texts = [open(p).read() for p in logs]
    names = [re.findall(r"Function Name: (\S+)", t) for t in texts]
    assert [len(n) for n in names[:6]] == [269, 36, 24, 48, 96, 24], [len(n) for n in names]
    assert len(names[6]) == 25 and len(set(sum(names, []))) == 269 + 36 + 24 + 48 + 96 + 24 + 25
    assert all("depth_kernel" in n or "pick_finish_kernel" in n for n in names[6])
    assert not [n for n in sum(names[:6], []) if "depth_kernel" in n or "pick_finish" in n]
    key = lambda name: tuple(int(g) for g in re.search(ROWS, name).groups())      # noqa: E731
    mine = {key(n): v for n, v in _kernels(texts[6], r"\d+depth_kernel" + ROWS.replace("(", "(?:")).items()}
    twins = {key(n): v for n, v in _kernels(texts[0], r"\d+mip_clipped" + ROWS.replace("(", "(?:")).items()}
    iso_rows = {key(n) for n in names[0] if re.search(r"\d+iso_clipped" + ROWS, n)}
    assert len(mine) == 24 and set(mine) == iso_rows and set(mine) <= set(twins)
    for row, (sgprs, vgprs, scratch, occupancy, sspill, vspill) in mine.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (row, scratch, sspill, vspill)
        assert twins[row][0] <= 80 and twins[row][1] <= 64, (row, twins[row])
        assert sgprs <= 80 and vgprs <= 64 and occupancy == 8, (row, sgprs, vgprs, occupancy)


def test_binding_and_header(vr):
    """vr_depth is 8 bytes (opacity, mode at 0 / 4), vr_depth_out 24 (three pointers), vr_pick 40 (hit, k, position, voxel, value, alpha at
    0 / 4 / 8 / 20 / 32 / 36); vr_params keeps its 132 bytes, VrLaunchInfo its 13 members and 52 bytes; the four entry points are
    declared in include/vr_hip.h, exported and resolved by the binding; without a context they return VR_ERR_INVALID; the renderer has the
    methods, the device list does not."""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    L = vr.lib()
    raw = C.CDLL(vr.library_path())
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert hasattr(L, name) and hasattr(raw, name), name
    assert re.search(r"typedef struct vr_depth \{\s*float\s+opacity;\s*uint32_t\s+mode;\s*\} vr_depth;", text)
    assert re.search(r"typedef struct vr_depth_out \{\s*void \*depth;\s*void \*value;\s*void \*alpha;\s*\} vr_depth_out;", text)
    assert re.search(r"typedef struct vr_pick \{\s*uint32_t\s+hit;\s*float\s+k;\s*float\s+position\[3\];\s*float\s+voxel\[3\];\s*float\s+value;\s*float\s+alpha;\s*\} vr_pick;", text)
    assert re.search(r"VR_DEPTH_FIRST = 0, VR_DEPTH_PEAK = 1, VR_DEPTH_MEAN = 2", text)
    D, O, P = vr.VrDepth, vr.VrDepthOut, vr.VrPick
    assert C.sizeof(D) == 8 and (D.opacity.offset, D.mode.offset) == (0, 4)
    assert C.sizeof(O) == 24 and (O.depth.offset, O.value.offset, O.alpha.offset) == (0, 8, 16)
    assert C.sizeof(P) == 40 and (P.hit.offset, P.k.offset, P.position.offset, P.voxel.offset, P.value.offset, P.alpha.offset) == (0, 4, 8, 20, 32, 36)
    assert C.sizeof(vr.VrParams) == 132 and len(vr.VrLaunchInfo._fields_) == 13 and C.sizeof(vr.VrLaunchInfo) == 52
    p, d, count = vr.VrParams(), vr.VrDepth(0.5, 0), C.c_uint64(0)
    buf = (C.c_float * 16)()
    out = vr.VrDepthOut(C.addressof(buf), None, None)
    xy, picked = (C.c_uint32 * 2)(0, 0), (vr.VrPick * 1)()
    assert L.vr_hip_render_depth(None, C.byref(p), C.byref(d), C.byref(out)) == 1
    assert L.vr_hip_render_depth_device(None, C.byref(p), C.byref(d), C.byref(out), None) == 1
    assert L.vr_hip_pick(None, C.byref(p), C.byref(d), 1, xy, picked) == 1
    assert L.vr_hip_depth_frames(None, C.byref(count)) == 1
    for method in ("render_depth", "render_depth_device", "pick", "depth_frames"):
        assert callable(getattr(vr.HipRenderer, method)), method
        assert not hasattr(vr.MultiRenderer, method), method       # single device: the device list stays without them
