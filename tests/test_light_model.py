"""CPU tier of the gradient lighting (include/vr_hip.h vr_hip_set_lighting): light_render of tests/feature_ref.c — the frames the GPU tier expects —
tied to the pinned restatement of the clipped composite (clip_render_ray, a text of its own), held against the geometry of three ramps, shown to be monotone in the shininess and to be
neither trivial nor the cue-lit frame on what the GPU tier renders; the register figures of the built composite_lit kernels; the layout of
VrLighting."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clip_helpers import CLIPS, IDENTITY, ClipRef, composite_params
from light_helpers import IDENTITY_LIGHTING, LIT_VOLUMES, PHONG, LightRef, cue, lit_views, lit_volumes, plateau


def test_identity_lighting_is_the_unlit_clipped_composite_on_every_golden_case(golden):
    """{ 1, 0, 0, 4 }: m = fma(0, sd, 1) = 1 and spec = (0 * sp) * c.w = 0, so fma(c, 1, 0) = c — light_render (the feature ray of
    tests/feature_ref.c) is clip_render (clip_render_ray) with light_kd = 0, byte for byte, under the identity clip and each of CLIPS, TRILINEAR and Q8, on every golden case
    that carries a frame.  (4 184 769 non-transparent pixels compared on this tree.)"""
    ref, clip_ref = LightRef.instance(), ClipRef.instance()
    checked = 0
    for case in golden.cases(True):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        for sampling in (1, 2):
            p = golden.params(case, sampling)
            for clip_name, clip in (("identity", IDENTITY),) + tuple(sorted(CLIPS.items())):
                want = clip_ref.composite(cue(p), vox, st["tf"], st["esl"], clip)
                assert np.array_equal(ref.render(p, vox, st["tf"], st["esl"], IDENTITY_LIGHTING, clip=clip), want), (case["label"], sampling, clip_name)
                checked += int((want[..., 3] != 0).sum())
    print("non-transparent pixels compared:", checked)
    assert checked > 100000, checked


def test_alpha_is_untouched_on_every_golden_case(golden):
    """Step 4 never writes c.w: the alpha plane under { 0.25, 0.65, 0.4, 4 } equals the cue-lit frame's on every golden case with a frame,
    both samplings; the colours differ on a good part of them (12-37 % of the pixels by the highlight alone)."""
    ref, clip_ref = LightRef.instance(), ClipRef.instance()
    differ = 0
    for case in golden.cases(True):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        for sampling in (1, 2):
            p = golden.params(case, sampling)
            lit, plain = ref.render(p, vox, st["tf"], st["esl"], PHONG), clip_ref.composite(p, vox, st["tf"], st["esl"], IDENTITY)
            assert np.array_equal(lit[..., 3], plain[..., 3]), (case["label"], sampling)
            differ += int((lit != plain).any(axis=-1).sum())
    assert differ > 10000, differ


def _ramp(axis):
    """32^3 u8, value 8 * i along x (axis 0), y (1) or z (2); arrays are indexed [z, y, x]"""
    shape = [1, 1, 1]
    shape[2 - axis] = 32
    return np.ascontiguousarray(np.broadcast_to((np.arange(32, dtype=np.uint8) * 8).reshape(shape), (32, 32, 32)))


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_ramp_geometry(vr, golden, oracle, axis):
    """A ramp's gradient lies along its axis exactly (a lerp of equal values is exact), so with diffuse only { 0, 1, 0, 0 }:
    the light at +-1000 on the ramp's axis gives sd >= 999 / sqrt(999^2 + 2) > 1 - 1.1e-6 for BOTH signs (two-sided) — every byte is within
    1 of the frame with light_kd = 0; the light at 1000 on a perpendicular axis gives sd <= 1 / 999 — every byte is within 1 of the
    { 0, 0, 0, 0 } frame (which is not black: samples with c.w <= 0.05 are never lit and keep their colour).  Both follow from
    256 * 0.002 < 1; neither is tuned.  Full march, Bucky's transfer function, the nine views, both samplings.
    (Worst on this tree, each of the three ramps: 1 byte along, 1 byte across.)"""
    ref, clip_ref, vox = LightRef.instance(), ClipRef.instance(), _ramp(axis)
    worst_along = worst_across = lit_bytes = 0
    for label, view in lit_views(vr, golden, "bucky"):
        for sampling in (1, 2):
            p, tf, esl = composite_params(vr, golden, oracle, "bucky", vox, view, sampling, True)
            unlit = clip_ref.composite(cue(p), vox, tf, esl, IDENTITY)
            for sign in (1.0, -1.0):
                q = p.copy()
                for j in range(3):
                    q.view.light_pos[j] = 1000.0 * sign if j == axis else 0.0
                out = ref.render(q, vox, tf, esl, (0.0, 1.0, 0.0, 0))
                worst_along = max(worst_along, int(np.abs(out.astype(int) - unlit.astype(int)).max()))
            q = p.copy()
            for j in range(3):
                q.view.light_pos[j] = 1000.0 if j == (axis + 1) % 3 else 0.0
            out, dark = ref.render(q, vox, tf, esl, (0.0, 1.0, 0.0, 0)), ref.render(q, vox, tf, esl, (0.0, 0.0, 0.0, 0))
            worst_across = max(worst_across, int(np.abs(out.astype(int) - dark.astype(int)).max()))
            assert np.array_equal(out[..., 3], unlit[..., 3])
            lit_bytes += int(unlit[..., :3].max())
    print("ramp along", "xyz"[axis], ": worst |byte - unlit byte| with the light along the ramp", worst_along, ", across", worst_across)
    assert worst_along <= 1 and worst_across <= 1, (worst_along, worst_across)
    assert lit_bytes > 18 * 50                       # the unlit frames are not dark: the bounds say something


def test_shininess_is_monotone(vr, golden, oracle):
    """Exact: sp <= 1, so squaring it once more never raises it; every later operation (ks * sp, * c.w, fma(c, m, spec), fma(c, t, acc) with
    t = 1 - acc.w >= 0 while a ray marches, map_float_int) is monotone and alpha never depends on it — for shininess_log2 = 0..7 under
    { 0.2, 0.5, 0.8 } no RGB byte rises from one value to the next and the alpha plane does not change.  Bucky, the nine views, default mode."""
    ref = LightRef.instance()
    vox = np.ascontiguousarray(golden.voxels("bucky"))
    fell = 0
    for label, view in lit_views(vr, golden, "bucky"):
        p, tf, esl = composite_params(vr, golden, oracle, "bucky", vox, view, 1, False)
        prev = None
        for n in range(8):
            out = ref.render(p, vox, tf, esl, (0.2, 0.5, 0.8, n))
            if prev is not None:
                assert (out[..., :3] <= prev[..., :3]).all() and np.array_equal(out[..., 3], prev[..., 3]), (label, n)
                fell += int((out[..., :3] < prev[..., :3]).sum())
            prev = out
    assert fell > 10000, fell


def test_gpu_tier_frames_are_neither_trivial_nor_the_cue(vr, golden, oracle):
    """The caps, conditions and not measurements.  For every scene the GPU tier renders, summed over its nine views: at least 5 % of the
    pixels are non-zero, at least 5 % differ from the cue-lit restatement, and at least 5 % differ between specular 0.4 and 0 — the GPU tier
    cannot pass on frames the lighting does not reach.  For the plateau volume at least 5 % of the dense samples take the !(gg > 0) branch
    and at least 5 % do not; on the other three volumes that branch is never taken, which is why the plateau is among them.
    (On this tree, default mode, non-zero / differ from the cue / differ by the highlight: bucky 51.5 / 51.1 / 27.0 %, blob_40x24x56
    34.6 / 34.0 / 18.3 %, random_u16 75.7 / 75.7 / 46.3 %, plateau 19.4 / 19.4 / 8.2 %; the plateau's zero-gradient share 9.6 % of 46 000
    dense samples — early termination ends most rays before the block's inside.)"""
    ref, clip_ref, volumes = LightRef.instance(), ClipRef.instance(), lit_volumes(golden)
    for name in LIT_VOLUMES:
        vox = volumes[name]
        nonzero = differ = highlight = pixels = dense = flat = 0
        for label, view in lit_views(vr, golden, name):
            p, tf, esl = composite_params(vr, golden, oracle, name, vox, view, 1, False)
            lit, d, f = ref.render(p, vox, tf, esl, PHONG, counters=True)
            dull = ref.render(p, vox, tf, esl, (PHONG[0], PHONG[1], 0.0, PHONG[3]))
            plain = clip_ref.composite(p, vox, tf, esl, IDENTITY)
            nonzero += int(lit.any(axis=-1).sum())
            differ += int((lit != plain).any(axis=-1).sum())
            highlight += int((lit != dull).any(axis=-1).sum())
            pixels += lit.shape[0] * lit.shape[1]
            dense += d
            flat += f
        print(f"{name}: {100 * nonzero / pixels:.1f} % of the pixels non-zero, {100 * differ / pixels:.1f} % differ from the cue-lit frame, "
              f"{100 * highlight / pixels:.1f} % differ by the highlight; {dense} dense samples, {100 * flat / max(dense, 1):.1f} % with a zero gradient")
        assert nonzero >= 0.05 * pixels and differ >= 0.05 * pixels and highlight >= 0.05 * pixels, (name, nonzero, differ, highlight, pixels)
        if name == "plateau":
            assert flat >= 0.05 * dense and dense - flat >= 0.05 * dense, (dense, flat)
    assert plateau().shape == (24, 24, 24) and int(plateau().max()) == 200


def _kernels(text, pattern):
    out = {}
    for m in re.finditer(r"Function Name: (\S*?" + pattern + r"\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        out[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    return out


def test_lit_kernels_keep_their_registers(vr):
    """Every composite_lit instantiation of the build: no scratch, no SGPR or VGPR spilled, at most 64 VGPRs and 96 SGPRs, 8 waves per SIMD
    (DESIGN.md section 4.8 has the table).  They exist for exactly the (SAMPLING, BPV, ADDR, LAYOUT) rows of raymarch_shadowed, 24 of them.
    The figures come from resource_usage_light.log, the lighting unit's own log next to resource_usage.log and resource_usage_shadow.log
    (csrc/Makefile); every name occurs once over the three logs, and the 24 of the lighting unit in no other."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    logs = [os.path.join(csrc, n) for n in ("resource_usage.log", "resource_usage_shadow.log", "resource_usage_light.log")]
    if not all(os.path.exists(p) for p in logs):
        subprocess.check_call(["make", "-B", "-C", csrc])
    text, shadow_text, light_text = (open(p).read() for p in logs)
    names, shadow_names, light_names = (re.findall(r"Function Name: (\S+)", t) for t in (text, shadow_text, light_text))
    assert len(light_names) == 24 and len(set(names + shadow_names + light_names)) == len(names) + len(shadow_names) + 24, (len(names), len(shadow_names), len(light_names))
    assert all("composite_lit" in n for n in light_names) and not [n for n in names + shadow_names if "composite_lit" in n]
    for taken in ("raymarch_kernel", "mip_kernel", "iso_kernel", "raymarch_clipped", "shadow"):      # what the existing register tests match on
        assert not [n for n in light_names if taken in n], taken
    lit = _kernels(light_text, r"composite_litILi(?:\d)ELi(?:\d)ELi(?:\d)ELi(?:\d)E")
    assert len(lit) == 24
    for name, (sgprs, vgprs, scratch, occupancy, sspill, vspill) in lit.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (name, scratch, sspill, vspill)
        assert vgprs <= 64 and sgprs <= 96 and occupancy == 8, (name, sgprs, vgprs, occupancy)
    key = lambda name: tuple(int(g) for g in re.search(r"ILi(\d)ELi(\d)ELi(\d)ELi(\d)E", name).groups())      # noqa: E731
    shadowed = {key(n) for n in shadow_names if "raymarch_shadowed" in n}
    assert {key(n) for n in lit} == shadowed and len(shadowed) == 24, sorted(lit)


def test_struct_layouts_match_the_header(vr):
    """VrLighting against vr_lighting of include/vr_hip.h (members, order, 16 bytes at offsets 0 / 4 / 8 / 12); vr_params keeps its 132
    bytes — the lighting is context state —; VrLaunchInfo is unchanged (13 members, 52 bytes); the three entry points are declared and bound"""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vr_lighting \{(.*?)\} vr_lighting;", text, flags=re.S).group(1)
    members = re.findall(r"(float|uint32_t)\s+(\w+);", body)
    assert members == [("float", "ambient"), ("float", "diffuse"), ("float", "specular"), ("uint32_t", "shininess_log2")]
    assert [n for n, _ in vr.VrLighting._fields_] == [m[1] for m in members]
    assert C.sizeof(vr.VrLighting) == 16
    assert [getattr(vr.VrLighting, m[1]).offset for m in members] == [0, 4, 8, 12]
    assert vr.VrLighting.ambient.size == 4 and vr.VrLighting.shininess_log2.size == 4
    assert C.sizeof(vr.VrParams) == 132
    body = re.search(r"typedef struct vr_launch_info \{(.*?)\} vr_launch_info;", text, flags=re.S).group(1)
    names = [n for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in vr.VrLaunchInfo._fields_] and names[-1] == "shadowed" and len(names) == 13 and C.sizeof(vr.VrLaunchInfo) == 52
    for name in ("vr_hip_set_lighting", "vr_hip_multi_set_lighting", "vr_hip_lighting_frames"):
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert hasattr(vr.lib(), name), name
