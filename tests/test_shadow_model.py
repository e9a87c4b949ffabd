"""CPU tier of the light-source shadows (include/vr_hip.h vr_hip_set_shadow): shadow_build and shadow_render of tests/feature_ref.c — the light grids
and frames the GPU tier expects — tied to the pinned restatement of the clipped composite, clip_render_ray, a text of its own, held against the geometry of an opaque shell, and
shown to be neither trivial nor unshadowed on what the GPU tier renders; the register figures of the built shadow kernels; the layout of
VrShadow and VrLaunchInfo."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clip_helpers import CLIPS, IDENTITY, ClipRef, composite_params
from iso_helpers import all_volumes, views_for
from shadow_helpers import COMPOSITE_VOLUMES, CUTOFF, FRAME_SCENES, GRID_SCENES, LIGHTS, SMALLEST, ShadowRef


def _state(golden, oracle, name, vox):
    """(tf, ray_step) of a volume: the golden state, or the oracle's scene for the synthetic ones"""
    p, tf, esl = composite_params(_state.vr, golden, oracle, name, vox, _state.vr.benchmark_view(80, 80, 0), 1, False)
    return tf, float(p.ray_step)


@pytest.fixture(autouse=True)
def _package(vr):
    _state.vr = vr


def test_shadow_off_is_the_clipped_composite_on_every_golden_case(golden):
    """Without a grid, and with a grid at strength 0 (f = fma(0, Tq, 1) = 1), shadow_render (the feature ray of tests/feature_ref.c) is clip_render (clip_render_ray) byte for byte:
    under the identity clip and under each of CLIPS, TRILINEAR and Q8, on every golden case that carries a frame"""
    ref, clip_ref = ShadowRef.instance(), ClipRef.instance()
    rng = np.random.default_rng(3)
    grid = rng.integers(0, 256, size=(5, 5, 5), dtype=np.uint8)          # any grid: strength 0 must not let it through
    checked = 0
    for case in golden.cases(True):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        for sampling in (1, 2):
            p = golden.params(case, sampling)
            for clip_name, clip in (("identity", IDENTITY),) + tuple(sorted(CLIPS.items())):
                want = clip_ref.composite(p, vox, st["tf"], st["esl"], clip)
                assert np.array_equal(ref.render(p, vox, st["tf"], st["esl"], None, 1.0, clip), want), (case["label"], sampling, clip_name, "no grid")
                assert np.array_equal(ref.render(p, vox, st["tf"], st["esl"], grid, 0.0, clip), want), (case["label"], sampling, clip_name, "strength 0")
                checked += int((want[..., 3] != 0).sum())
    assert checked > 100000, checked


def test_a_uniform_grid_scales_the_unlit_dense_colour(vr, golden, oracle):
    """A grid of 255 everywhere at strength 1 is f = 1: the plain frame.  A grid of 0 everywhere leaves alpha alone and darkens the colour."""
    ref, vox = ShadowRef.instance(), np.ascontiguousarray(golden.voxels("bucky"))
    p, tf, esl = composite_params(vr, golden, oracle, "bucky", vox, vr.benchmark_view(80, 80, 1), 1, True)
    plain = ref.render(p, vox, tf, esl)
    assert np.array_equal(ref.render(p, vox, tf, esl, np.full((9, 9, 9), 255, np.uint8), 1.0), plain)
    black = ref.render(p, vox, tf, esl, np.zeros((9, 9, 9), np.uint8), 1.0)
    assert np.array_equal(black[..., 3], plain[..., 3]) and (black[..., :3] <= plain[..., :3]).all() and black[..., :3].sum() < 0.5 * plain[..., :3].sum()


def test_geometry_of_the_grid_on_the_opaque_shell(golden, oracle):
    """shell48 (oracle/vr_oracle.c vro_generate_volume kind 0) is a wall around radius 0.6: its value without the noise of 0..15 is above 0
    only for radii in (0.346, 0.775), and at least 100 for radii in [0.4637, 0.7106].  Light at (0, 0, 3), S = 17.
    (1) A node whose segment to the light stays farther than 0.775 + 0.08 from the centre — a voxel diagonal is 0.072 — meets only noise,
        which the default transfer function maps to alpha 0: q == 255.
    (2) A node at z <= 0 whose segment passes within 0.5 of the centre, at or behind the node, crosses all of the radii 0.536 .. 0.638 on
        its way out: there all eight corners of a sample's cell lie in the band of values >= 100 (0.4637 + 0.0722, 0.7106 - 0.0722), the
        radius changes by at most `step` per sample, so at least floor(0.102 / step) samples have an alpha of at least the smallest alpha
        the transfer function gives a raw value >= 100 — in double precision, over its entries from floor(100 * 128 / 255 - 0.5) on.  q is
        at most 255 times that power, rounded up.
    (3) The node at the light itself, the nodes of the face z = +1, whose light rays point out of the cube, and a light inside the cube"""
    ref, vox = ShadowRef.instance(), np.ascontiguousarray(golden.voxels("shell48"))
    tf, step = _state(golden, oracle, "shell48", vox)
    S, light = 17, np.array(LIGHTS["top"], np.float64)
    q = ref.build(LIGHTS["top"], S, step, vox, tf)
    g = np.linspace(-1.0, 1.0, S)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    nodes = np.stack([xx, yy, zz], axis=-1)
    d = light - nodes
    t_star = np.clip(-(nodes * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)            # closest approach of the segment node -> light to the centre
    closest = np.linalg.norm(nodes + d * t_star[..., None], axis=-1)
    far = closest > 0.775 + 0.08
    assert far.sum() > 500 and (q[far] == 255).all(), (int(far.sum()), int((q[far] != 255).sum()))
    first = int(np.floor(100.0 * 128.0 / 255.0 - 0.5))
    alpha = float(np.asarray(tf, np.float64).reshape(128, 4)[first:, 3].min())
    samples = int(np.floor((0.638 - 0.536) / step))
    bound = int(np.ceil(255.0 * (1.0 - alpha) ** samples)) + 1
    free = -(nodes * d).sum(-1) / (d * d).sum(-1)
    behind = (zz <= 0.0) & (free >= 0.0) & (closest < 0.5)
    assert alpha > 0.05 and samples >= 1 and bound < 200, (alpha, samples, bound)          # a bound that says something
    assert behind.sum() > 100 and (q[behind] <= bound).all(), (int(behind.sum()), bound, int(q[behind].max()))
    assert (q[S - 1] == 255).all()                                               # the face z = +1: every light ray leaves the cube at once
    # (3a) the node at the light itself: len2 == 0, T = 1
    at_node = (0.25, -0.5, 0.0)                                                  # node (10, 4, 8) exactly
    assert ref.build(at_node, S, step, vox, tf)[8, 4, 10] == 255
    # (3b) faces pointing away from the cube towards the light: a node on a face whose light vector has a positive component along the
    # face's outward normal leaves the cube at t = 0 (ky = 0: intersect's miss) — under the outside light (2, 1.5, -2.5) the faces
    # x = +1, y = +1 and z = -1, whole
    q_out = ref.build(LIGHTS["outside"], S, step, vox, tf)
    assert (q_out[:, :, S - 1] == 255).all() and (q_out[:, S - 1, :] == 255).all() and (q_out[0] == 255).all()
    assert (q_out < 255).any()
    # (3c) a light inside the hollow, at radius 0.187.  A node whose whole segment to it stays inside radius 0.346 - 0.08 (the radius along
    # a segment is largest at one of its ends) meets only noise: q == 255.  A node at radius >= 0.638 crosses all of the band 0.536 .. 0.638
    # before its ray ends at the light: at most the bound of (2).
    hollow = (0.1, -0.05, 0.15)
    q_in = ref.build(hollow, S, step, vox, tf)
    r_node, r_light = np.linalg.norm(nodes, axis=-1), float(np.linalg.norm(hollow))
    clear = np.maximum(r_node, r_light) < 0.346 - 0.08
    walled = r_node >= 0.638
    assert r_light < 0.346 - 0.08 and clear.sum() >= 20 and (q_in[clear] == 255).all(), (int(clear.sum()), int((q_in[clear] != 255).sum()))
    assert walled.sum() > 3000 and (q_in[walled] <= bound).all(), (int(walled.sum()), bound, int(q_in[walled].max()))


def _grid(ref, golden, oracle, volumes, name, light, S):
    tf, step = _state(golden, oracle, name, volumes[name])
    return ref.build(LIGHTS[light], S, step, volumes[name], tf)


def test_gpu_tier_grids_and_frames_are_neither_trivial_nor_unshadowed(vr, golden, oracle):
    """The cap, a condition and not a measurement.  For every (volume, light, S) whose grid the GPU tier downloads at least 5 % of the nodes
    are neither 0 nor 255; for every scene whose frames it renders at least 5 % of the pixels, summed over the nine views of views_for, are
    non-zero and at least 5 % of the pixels differ from the unshadowed restatement: the GPU tier cannot pass on grids of one value or on
    frames the shadow does not reach.  SMALLEST, the grid of the cube's eight corners, is held to the same three conditions: 5 % of 8 nodes
    is one corner byte strictly between 0 and 255."""
    ref, volumes = ShadowRef.instance(), all_volumes(golden)
    for name, light, S in GRID_SCENES + (SMALLEST,):
        q = _grid(ref, golden, oracle, volumes, name, light, S)
        between = int(((q != 0) & (q != 255)).sum())
        print(f"{name} {light} S={S}: {100 * between / q.size:.1f} % of the nodes neither 0 nor 255, {100 * (q == 0).mean():.1f} % black")
        assert between >= 0.05 * q.size, (name, light, S, between, q.size)
    print("smallest grid:", _grid(ref, golden, oracle, volumes, *SMALLEST).ravel().tolist())
    for name, light, S in sorted((n, l, s) for n, (l, s) in FRAME_SCENES.items()) + [SMALLEST]:
        q = _grid(ref, golden, oracle, volumes, name, light, S)
        nonzero = differ = pixels = 0
        for label, view in views_for(vr, golden, name):
            p, tf, esl = composite_params(vr, golden, oracle, name, volumes[name], view, 1, False)
            shadowed, plain = ref.render(p, volumes[name], tf, esl, q, 1.0), ref.render(p, volumes[name], tf, esl)
            nonzero += int(shadowed.any(axis=-1).sum())
            differ += int((shadowed != plain).any(axis=-1).sum())
            pixels += shadowed.shape[0] * shadowed.shape[1]
        print(f"{name} {light} S={S}: {100 * nonzero / pixels:.1f} % of the pixels non-zero, {100 * differ / pixels:.1f} % differ from the unshadowed frame")
        assert nonzero >= 0.05 * pixels and differ >= 0.05 * pixels, (name, light, S, nonzero, differ, pixels)
    assert set(FRAME_SCENES) == set(COMPOSITE_VOLUMES)


def test_the_cutoff_blackens_and_the_builder_sampling_matters(golden, oracle):
    """cutoff: every q below round(255 * cutoff) is 0 (a ray that fell below it is black), none with cutoff 0; the Q8 builder differs from
    the fp32 one in some node and nowhere by more than a few levels"""
    ref, volumes = ShadowRef.instance(), all_volumes(golden)
    vox = volumes["bucky"]
    tf, step = _state(golden, oracle, "bucky", vox)
    q = ref.build(LIGHTS["outside"], 17, step, vox, tf, cutoff=0.25)
    assert ((q == 0) | (q >= 63)).all() and (q == 0).any()
    q8 = ref.build(LIGHTS["outside"], 17, step, vox, tf, sampling=2)
    q1 = ref.build(LIGHTS["outside"], 17, step, vox, tf)
    delta = np.abs(q8.astype(np.int16) - q1.astype(np.int16))
    assert delta.any() and delta.max() <= 8, int(delta.max())
    assert CUTOFF == 1.0 / 256.0


def _kernels(text, pattern):
    out = {}
    for m in re.finditer(r"Function Name: (\S*?" + pattern + r"\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        out[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    return out


def test_shadow_kernels_keep_their_registers(vr):
    """Every raymarch_shadowed and shadow_build_kernel instantiation of the build: no scratch, no SGPR or VGPR spilled, at most 64 VGPRs and
    96 SGPRs, 8 waves per SIMD (DESIGN.md section 4.7 has the table).  The shadowed composite exists for exactly the TRILINEAR and Q8 rows of
    the clipped composite; the builder for the linear array, the quad and the oct bricks over all addressing paths.  The figures come from
    resource_usage_shadow.log, the shadow unit's own log next to resource_usage.log (csrc/Makefile: tests/test_abi.py pins the number of
    names in that one); every name occurs once over both logs, and the 36 of the shadow unit in no other."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    log = os.path.join(csrc, "resource_usage.log")
    if not os.path.exists(log):
        subprocess.check_call(["make", "-B", "-C", csrc])
    own = os.path.join(csrc, "resource_usage_shadow.log")
    if not os.path.exists(own):
        subprocess.check_call(["make", "-B", "-C", csrc])
    text, shadow_text = open(log).read(), open(own).read()
    names, shadow_names = re.findall(r"Function Name: (\S+)", text), re.findall(r"Function Name: (\S+)", shadow_text)
    assert len(shadow_names) == 36 and len(set(names + shadow_names)) == len(names) + 36, (len(names), len(shadow_names))
    assert not [n for n in names if "shadow" in n] and all("shadow" in n for n in shadow_names)
    shadowed = _kernels(shadow_text, r"raymarch_shadowedILi(?:\d)ELi(?:\d)ELi(?:\d)ELi(?:\d)E")
    builders = _kernels(shadow_text, r"shadow_build_kernelILi(?:\d)ELi(?:\d)ELi(?:\d)E")
    for name, (sgprs, vgprs, scratch, occupancy, sspill, vspill) in list(shadowed.items()) + list(builders.items()):
        assert scratch == 0 and sspill == 0 and vspill == 0, (name, scratch, sspill, vspill)
        assert vgprs <= 64 and sgprs <= 96 and occupancy == 8, (name, sgprs, vgprs, occupancy)
    key = lambda name, n: tuple(int(g) for g in re.search(r"ILi(\d)" + r"ELi(\d)" * (n - 1) + "E", name).groups())      # noqa: E731
    clipped = {key(n, 4) for n in re.findall(r"Function Name: (\S*raymarch_clippedILi\dELi\dELi\dELi\dE\S*)", text)}
    assert {key(n, 4) for n in shadowed} == {k for k in clipped if k[0] in (1, 2)} and len(shadowed) == 24, sorted(shadowed)
    assert {key(n, 3) for n in builders} == {k[1:] for k in clipped if k[0] == 1} and len(builders) == 12, sorted(builders)


def test_struct_layouts_match_the_header(vr):
    """VrShadow against vr_shadow of include/vr_hip.h (members, order, 32 bytes); vr_params keeps its 132 bytes — the shadow is context
    state —; VrLaunchInfo is the header's vr_launch_info, the twelve members it had and `shadowed` behind them"""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vr_shadow \{(.*?)\} vr_shadow;", text, flags=re.S).group(1)
    members = re.findall(r"(float|uint32_t)\s+(\w+)(?:\[(\d)\])?;", body)
    assert members == [("float", "light_pos", "3"), ("uint32_t", "dims", ""), ("float", "step", ""), ("float", "strength", ""), ("float", "cutoff", ""),
                       ("uint32_t", "sampling", "")]
    assert [n for n, _ in vr.VrShadow._fields_] == [m[1] for m in members]
    assert C.sizeof(vr.VrShadow) == 32
    assert [getattr(vr.VrShadow, m[1]).offset for m in members] == [0, 12, 16, 20, 24, 28]
    assert vr.VrShadow.dims.size == 4 and vr.VrShadow.light_pos.size == 12
    assert C.sizeof(vr.VrParams) == 132
    body = re.search(r"typedef struct vr_launch_info \{(.*?)\} vr_launch_info;", text, flags=re.S).group(1)
    names = [n for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in vr.VrLaunchInfo._fields_]
    assert names[-1] == "shadowed" and len(names) == 13 and C.sizeof(vr.VrLaunchInfo) == 12 * 4 + 4
    for name in ("vr_hip_set_shadow", "vr_hip_multi_set_shadow", "vr_hip_download_shadow", "vr_hip_shadow_builds"):
        assert re.search(r"\bint\s+" + name + r"\(", text), name
