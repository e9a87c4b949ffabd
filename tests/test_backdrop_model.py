"""CPU tier of the backdrop and hybrid frames (include/vr_hip.h vr_hip_render_backdrop / vr_hip_render_hybrid): backdrop_render and
hybrid_render of tests/feature_ref.c — the frames the GPU tier expects — tied to the pinned restatement of the composite (slab_render, and
through it the clipped, shadowed and gradient-lit ones) where there is no surface, shown to return the layer where nothing is composited,
to be non-trivial on the hybrids the GPU tier renders, and to be sensitive to three wrong readings of the contract on the GPU tier's own
frames; the register figures of the built backdrop kernels next to those of their twins; the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from backdrop_helpers import BACKDROP_VOLUMES, BYTE_OVER_255, HYBRID_LEVELS, K_LT_D, NO_BLEND_AFTER_ERT, BackdropRef, synthetic_layer, tier_frames
from clip_helpers import CLIPS, IDENTITY, ClipRef
from feature_random import generator
from light_helpers import PHONG
from light_helpers import lit_views as backdrop_views
from light_helpers import lit_volumes as backdrop_volumes
from shadow_helpers import LIGHTS, ShadowRef
from slab_helpers import POINT, SLAB, SlabRef
from slab_helpers import slab_scene as backdrop_scene

GRID_S = 9                                          # the light grid of the tie: small, and not uniform on any golden volume
NEW_SYMBOLS = ("vr_hip_render_backdrop_device", "vr_hip_render_backdrop", "vr_hip_render_hybrid_device", "vr_hip_render_hybrid", "vr_hip_backdrop_frames")


@pytest.fixture(autouse=True)
def feature_is_built(vr):
    """every test of this file is about the library's contract: without its entry points there is nothing to restate"""
    L = vr.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name


def diff(a, b):
    return int((a != b).any(axis=-1).sum())


def test_without_a_surface_the_frame_is_the_pinned_restatement(golden):
    """NULL layers, and a depth layer of all -1, all NaN, or negative values (random, -0.0 excluded, -inf included) under random colour
    words, give the bytes of slab_render: point and slab mode, every golden case that carries a frame (TRILINEAR and Q8 in turn), the identity clip
    and each of CLIPS, the cue alone and a lighting with a light grid.  backdrop_render and slab_render wrap one ray of
    tests/feature_ref.c: the tie shows that layers without a surface switch nothing on, not that two texts agree —
    tests/test_restatement_pins.py pins the single ray to the five texts it replaced."""
    ref, slab_ref, shadow_ref = BackdropRef.instance(), SlabRef.instance(), ShadowRef.instance()
    rng = generator(412)
    checked = turn = 0
    for index, case in enumerate(golden.cases(True)):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        tf, esl = st["tf"], st["esl"]
        for sampling in (1 + index % 2,):               # TRILINEAR and Q8 alternate over the cases
            p = golden.params(case, sampling)
            q = shadow_ref.build(LIGHTS["top"], GRID_S, p.ray_step, vox, tf)
            shape = (p.out_rows, p.out_width)
            rgba = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
            negative = -np.abs(rng.normal(size=shape)).astype(np.float32) - np.float32(1e-30)
            negative[rng.random(size=shape) < 0.1] = -np.inf
            layers = (np.full(shape, -1.0, np.float32), np.full(shape, np.nan, np.float32), negative)
            for clip_name, clip in (("identity", IDENTITY),) + tuple(sorted(CLIPS.items())):
                for mode in (POINT, SLAB):
                    for lighting, grid in ((None, None), (PHONG, q)):
                        what = (case["label"], sampling, clip_name, mode, lighting)
                        want = slab_ref.render(p, vox, tf, esl, mode, clip, lighting, grid, 0.6)
                        assert np.array_equal(ref.render(p, vox, tf, esl, None, None, mode, clip, lighting, grid, 0.6), want), what
                        depth = layers[turn % 3]                # the three kinds in turn: every kind meets every clip, mode and lighting over the cases
                        turn += 1
                        assert np.array_equal(ref.render(p, vox, tf, esl, rgba, depth, mode, clip, lighting, grid, 0.6), want), what
                        checked += int((want[..., 3] != 0).sum())
    print("non-transparent pixels compared:", checked)
    assert checked > 100000, checked


def _inside_depth(ref, p, vox, tf, esl):
    """per pixel the middle of the ray's segment through the cube; 1 where there is none"""
    seg = ref.segments(p, vox, tf, esl)
    return np.where(np.isnan(seg[..., 0]), np.float32(1.0), np.float32(0.5) * (seg[..., 0] + seg[..., 1])).astype(np.float32)


def test_a_transparent_volume_returns_the_colour_layer(vr, golden, oracle):
    """A transfer function of zeros: acc stays 0, t = 1, and (int) (256 * ((byte + 0.5) / 256)) == byte — the colour layer comes back bit
    for bit, whether the ray misses, is leapt empty or composites nothing.  All 256 byte values in every channel; depths +inf, 0 and
    inside the cube; default mode and full march, point and slab mode, the cue and a lighting."""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    zeros = np.zeros((128, 4), np.float32)
    frames = 0
    for name in ("bucky", "random_u16"):
        for label, view in backdrop_views(vr, golden, name)[:6]:
            for full_march in (False, True):
                vox, p, _, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 1, full_march)
                rgba, _ = synthetic_layer(ref, p, vox, zeros, esl, salt=7, all_bytes=True)
                for ch in range(4):
                    assert len(np.unique(rgba[..., ch])) == 256
                shape = (p.out_rows, p.out_width)
                for depth in (np.full(shape, np.inf, np.float32), np.zeros(shape, np.float32), _inside_depth(ref, p, vox, zeros, esl)):
                    for mode, lighting in ((POINT, None), (SLAB, PHONG)):
                        assert np.array_equal(ref.render(p, vox, zeros, esl, rgba, depth, mode, lighting=lighting), rgba), (name, label, full_march, mode)
                        frames += 1
    assert frames == 2 * 6 * 2 * 3 * 2


def test_a_depth_in_front_of_the_segment_gives_the_layer(vr, golden, oracle):
    """d < kx (half of kx: the benchmark cameras stand outside the cube, kx > 0) and d == 0: the narrowed segment is empty, the ray is a
    miss, the pixel is the layer's colour word — on pixels whose plain frame is not empty"""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    covered = 0
    for name in BACKDROP_VOLUMES:
        for label, view in backdrop_views(vr, golden, name)[:8]:
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 1, False)
            rgba, _ = synthetic_layer(ref, p, vox, tf, esl, salt=8)
            seg = ref.segments(p, vox, tf, esl)
            kx = seg[..., 0]
            assert np.nanmin(kx) > 0
            front = np.where(np.isnan(kx), np.float32(0.25), np.float32(0.5) * kx).astype(np.float32)
            for depth in (front, np.zeros_like(front)):
                assert np.array_equal(ref.render(p, vox, tf, esl, rgba, depth), rgba), (name, label)
            covered += int(ref.render(p, vox, tf, esl).any(axis=-1).sum())
    assert covered > 32 * 500, covered


def test_a_surface_behind_everything_is_a_background_image(vr, golden, oracle):
    """d = +inf narrows nothing.  Pixels the plain frame leaves empty (misses, fully empty rays) become the layer's colour word.  Where the
    plain frame's alpha byte is 255, acc.w >= 255 / 256, so t = 1 - acc.w <= 1 / 256 and bf * t < 1 / 256: no byte moves by more than 1.
    Everywhere else the pixel is the blend of the plain frame's accumulated colour: alpha never falls."""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    empty = opaque = 0
    for name in BACKDROP_VOLUMES:
        for label, view in backdrop_views(vr, golden, name):
            for full_march in (False, True):
                vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 2, full_march)
                rgba, _ = synthetic_layer(ref, p, vox, tf, esl, salt=9)
                plain = ref.render(p, vox, tf, esl)
                out = ref.render(p, vox, tf, esl, rgba, np.full(rgba.shape[:2], np.inf, np.float32))
                seg = ref.segments(p, vox, tf, esl)
                nothing = np.isnan(seg[..., 2])                 # a miss, or leaping left kx > ky
                assert not plain[nothing].any() and np.array_equal(out[nothing], rgba[nothing]), (name, label, full_march)
                solid = plain[..., 3] == 255
                assert np.abs(out[solid].astype(int) - plain[solid].astype(int)).max(initial=0) <= 1, (name, label, full_march)
                assert (out[~nothing][..., 3] >= plain[~nothing][..., 3]).all()
                empty, opaque = empty + int(nothing.sum()), opaque + int(solid.sum())
    print(f"{empty} empty pixels took the layer, {opaque} opaque pixels kept their colour")
    assert empty > 10000 and opaque > 10000, (empty, opaque)


def test_hybrid_is_the_isosurface_under_the_backdrop(vr, golden, oracle):
    """hybrid_render's isosurface frame and depth are clip_iso_render's (one frame function of tests/feature_ref.c), bits and bytes, under the identity clip and
    under `both`, at refine 0 and 4; and the hybrid is backdrop_render over them"""
    ref, clip_ref, volumes = BackdropRef.instance(), ClipRef.instance(), backdrop_volumes(golden)
    for name in BACKDROP_VOLUMES:
        for label, view in backdrop_views(vr, golden, name)[1:4]:
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 1, False)
            for clip in (IDENTITY, CLIPS["both"]):
                for refine in (0, 4):
                    out, depth, iso = ref.hybrid(p, vox, tf, esl, HYBRID_LEVELS[name], refine, clip=clip)
                    want_iso, want_depth, _ = clip_ref.iso(p, vox, tf, HYBRID_LEVELS[name], refine, clip)
                    assert np.array_equal(iso, want_iso) and np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), (name, label, refine)
                    assert np.array_equal(out, ref.render(p, vox, tf, esl, iso, depth, clip=clip)), (name, label, refine)


def test_gpu_tier_hybrids_are_not_trivial(vr, golden, oracle):
    """Conditions, not measurements, per volume of the GPU tier at its level of HYBRID_LEVELS, nine views, default mode: at least a fifth of
    the non-empty pixels have a surface; of those at least a fifth differ from the isosurface frame's bytes (the volume in front
    contributes) and at least a fifth from the plain composite's (the march really stopped).
    (On this tree, surface / differs from the isosurface / differs from the composite: bucky 0.65 / 0.96 / 1.00, blob_40x24x56 0.47 / 1.00 /
    1.00, random_u16 0.98 / 0.51 / 1.00, plateau 0.84 / 0.99 / 1.00 — DESIGN.md section 4.11.)"""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    for name in BACKDROP_VOLUMES:
        nonempty = surface = not_iso = not_plain = 0
        for label, view in backdrop_views(vr, golden, name):
            vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, name, view, 1, False)
            out, depth, iso = ref.hybrid(p, vox, tf, esl, HYBRID_LEVELS[name], 4)
            plain = ref.render(p, vox, tf, esl)
            has = depth >= 0
            nonempty += int((out.any(axis=-1) | plain.any(axis=-1)).sum())
            surface += int(has.sum())
            not_iso += int(((out != iso).any(axis=-1) & has).sum())
            not_plain += int(((out != plain).any(axis=-1) & has).sum())
        print(f"{name} at level {HYBRID_LEVELS[name]}: {surface} of {nonempty} non-empty pixels have a surface ({surface / max(nonempty, 1):.2f}); "
              f"{not_iso / max(surface, 1):.2f} of those differ from the isosurface frame, {not_plain / max(surface, 1):.2f} from the plain composite")
        assert nonempty > 2000 and surface >= 0.2 * nonempty, (name, surface, nonempty)
        assert not_iso >= 0.2 * surface and not_plain >= 0.2 * surface, (name, not_iso, not_plain, surface)


def test_gpu_tier_frames_tell_three_wrong_readings_apart(vr, golden, oracle):
    """Sensitivity.  The restatement perturbed three ways — a sample at k == d not composited (`k < d`), the layer not blended in once early
    termination has struck, bf = byte / 255 — over the 864 frames of the GPU tier's main test (tier_frames: four volumes, both samplings,
    nine views, three marches, two steps, cue on and off), each with its synthetic layer: more than half of the frames change under each.
    The second reading can only show where a ray terminates early, which the full march (threshold 1) never does: the tier has the march
    `ert` (no leaping, threshold 0.95) beside the default mode for that.
    (On this tree: 864 / 504 / 864 of 864.)"""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    frames = 0
    changed = {K_LT_D: 0, NO_BLEND_AFTER_ERT: 0, BYTE_OVER_255: 0}
    for name in BACKDROP_VOLUMES:
        for sampling in (1, 2):
            for what, vox, p, tf, esl, rgba, depth in tier_frames(vr, golden, oracle, volumes, name, sampling):
                want = ref.render(p, vox, tf, esl, rgba, depth)
                frames += 1
                for perturb in changed:
                    changed[perturb] += int(not np.array_equal(want, ref.render(p, vox, tf, esl, rgba, depth, perturb=perturb)))
    print(f"of {frames} frames: {changed[K_LT_D]} change under k < d, {changed[NO_BLEND_AFTER_ERT]} without the blend after early termination, "
          f"{changed[BYTE_OVER_255]} under byte / 255")
    assert frames == 864
    for perturb, n in changed.items():
        assert 2 * n > frames, (perturb, n, frames)


def test_synthetic_layers_hold_every_kind_of_depth(vr, golden, oracle):
    """the generator's mix on a frame of the GPU tier: -1, NaN, 0, +inf, before kx, inside the segment, beyond ky, and exactly on a sample"""
    ref, volumes = BackdropRef.instance(), backdrop_volumes(golden)
    vox, p, tf, esl = backdrop_scene(vr, golden, oracle, volumes, "bucky", backdrop_views(vr, golden, "bucky")[1][1], 1, True)
    rgba, depth = synthetic_layer(ref, p, vox, tf, esl, salt=3)
    seg = ref.segments(p, vox, tf, esl)
    kx, ky, k0 = seg[..., 0], seg[..., 1], seg[..., 2]
    have = ~np.isnan(kx)
    with np.errstate(invalid="ignore"):
        counts = [int((depth == -1).sum()), int(np.isnan(depth).sum()), int((depth == 0).sum()), int(np.isposinf(depth).sum()),
                  int((have & (depth > 0) & (depth < kx)).sum()), int((have & (depth >= kx) & (depth <= ky)).sum()), int((have & (depth > ky) & np.isfinite(depth)).sum())]
        step = np.float32(p.ray_step)
        n = np.rint((depth - k0) / step)
        on = have & np.isfinite(depth) & (depth >= k0) & (n >= 1)
    from backdrop_helpers import sample_ks
    exact = on & (sample_ks(np.where(on, k0, 0), step, np.where(on, n, 0).astype(np.int64)) == depth)
    counts.append(int(exact.sum()))
    print("depth kinds:", counts)
    assert all(c >= 100 for c in counts), counts


def _kernels(text, pattern):
    out = {}
    for m in re.finditer(r"Function Name: (\S*?" + pattern + r"\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S):
        out[m.group(1)] = tuple(int(g) for g in m.groups()[1:])
    return out


# family -> (its twin without a backdrop, the log the twin's figures are in, the most VGPRs of the family's 24 rows)
FAMILIES = {"composite_backdrop": ("raymarch_shadowed", 1, 64), "composite_backdrop_lit": ("composite_lit", 2, 64),
            "composite_backdrop_slab": ("composite_slab", 3, 82), "composite_backdrop_slab_lit": ("composite_slab_lit", 3, 80)}
ROWS = r"ILi(\d)ELi(\d)ELi(\d)ELi(\d)E"


def test_backdrop_kernels_keep_their_twins_registers(vr):
    """The fifth log, resource_usage_backdrop.log: 96 names, each once and in no other log — four families over the 24 rows of
    composite_lit.  No scratch, no SGPR or VGPR spilled.  The goal, the VGPRs of the twin without a backdrop, is reached on every row:
    each kernel takes at most the VGPRs and SGPRs of its twin of the same (SAMPLING, BPV, ADDR, LAYOUT) and keeps at least its occupancy —
    composite_backdrop against raymarch_shadowed, composite_backdrop_lit against composite_lit, the slab families against composite_slab
    and composite_slab_lit.  (The pixel's element index is the one register the layer adds across the march, and it replaces the two of
    the output address.)  The other four logs keep their 269 / 36 / 24 / 48 names."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    logs = [os.path.join(csrc, n) for n in ("resource_usage.log", "resource_usage_shadow.log", "resource_usage_light.log", "resource_usage_slab.log",
                                            "resource_usage_backdrop.log")]
    if not all(os.path.exists(p) for p in logs):
        subprocess.check_call(["make", "-B", "-C", csrc])
    texts = [open(p).read() for p in logs]
    names = [re.findall(r"Function Name: (\S+)", t) for t in texts]
    assert [len(n) for n in names] == [269, 36, 24, 48, 96], [len(n) for n in names]
    assert len(set(sum(names, []))) == 269 + 36 + 24 + 48 + 96
    assert all("composite_backdrop" in n for n in names[4]) and not [n for n in sum(names[:4], []) if "backdrop" in n]
    key = lambda name: tuple(int(g) for g in re.search(ROWS, name).groups())      # noqa: E731
    lit_rows = {key(n) for n in names[2]}
    assert len(lit_rows) == 24
    for family, (twin, log, most_vgprs) in FAMILIES.items():
        mine = {key(n): v for n, v in _kernels(texts[4], r"\d" + family + ROWS.replace("(", "(?:")).items()}
        theirs = {key(n): v for n, v in _kernels(texts[log], r"\d" + twin + ROWS.replace("(", "(?:")).items()}
        assert set(mine) == lit_rows and set(mine) <= set(theirs), (family, len(mine), len(theirs))
        for row, (sgprs, vgprs, scratch, occupancy, sspill, vspill) in mine.items():
            t_sgprs, t_vgprs, _, t_occupancy, _, _ = theirs[row]
            assert scratch == 0 and sspill == 0 and vspill == 0, (family, row, scratch, sspill, vspill)
            assert vgprs <= t_vgprs and sgprs <= t_sgprs and occupancy >= t_occupancy, (family, row, (sgprs, vgprs, occupancy), theirs[row])
            assert vgprs <= most_vgprs, (family, row, vgprs)


def test_binding_and_header(vr):
    """vr_backdrop is 16 bytes; vr_params keeps its 132, VrLaunchInfo its 13 members and 52 bytes; the five entry points are declared in
    include/vr_hip.h, exported and resolved by the binding; without a context they return VR_ERR_INVALID; the renderer has the methods."""
    from test_abi import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vr_hip.h")).read(), flags=re.S)
    L = vr.lib()
    raw = C.CDLL(vr.library_path())
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert hasattr(L, name) and hasattr(raw, name), name
    assert re.search(r"typedef struct vr_backdrop \{\s*const void \*rgba;\s*const void \*depth;\s*\} vr_backdrop;", text)
    assert C.sizeof(vr.VrBackdrop) == 16 and vr.VrBackdrop.depth.offset == 8
    assert C.sizeof(vr.VrParams) == 132 and len(vr.VrLaunchInfo._fields_) == 13 and C.sizeof(vr.VrLaunchInfo) == 52
    p, layer, iso, count = vr.VrParams(), vr.VrBackdrop(), vr.VrIso(100.0, 4), C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    assert L.vr_hip_render_backdrop(None, C.byref(p), C.byref(layer), buf) == 1
    assert L.vr_hip_render_backdrop_device(None, C.byref(p), C.byref(layer), buf, None) == 1
    assert L.vr_hip_render_hybrid(None, C.byref(p), C.byref(iso), buf, None) == 1
    assert L.vr_hip_render_hybrid_device(None, C.byref(p), C.byref(iso), buf, None, None) == 1
    assert L.vr_hip_backdrop_frames(None, C.byref(count)) == 1
    for method in ("render_backdrop", "render_backdrop_device", "render_hybrid", "render_hybrid_device", "backdrop_frames"):
        assert callable(getattr(vr.HipRenderer, method)), method
    assert not hasattr(vr.MultiRenderer, "render_backdrop")        # single device: the device list stays without it
