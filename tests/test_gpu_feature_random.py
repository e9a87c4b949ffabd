"""Randomised and ragged-volume parity of the newer render features: the clipped composite, the MIP, the isosurface with depth, the light
grid, the shadowed and the gradient-lit frames on the random volumes and views of tests/test_gpu_random.py (odd extents, an extent of
1 / 2 / 8 / 16 / 33, cameras inside the cube, exact zeros in the direction, the four-fold ray step) under a random clip, light, grid size,
lighting and level per frame, and on the hand-made EDGE_SHAPES — every byte equal to the restatements tests/clip_ref.c, shadow_ref.c and
light_ref.c.  tests/feature_random.py draws the frames; tests/test_feature_random_model.py ties the restatements to one another on them
and shows that they are neither empty nor untouched by the feature.  Other seeds: VR_TEST_SEED=... pytest -m gpu tests/test_gpu_feature_random.py"""
import os
import subprocess
import sys

import numpy as np
import pytest

import feature_random as fr
from clip_helpers import ClipRef, set_clip
from helpers import ROOT
from iso_helpers import depth_bits
from light_helpers import LightRef
from shadow_helpers import CUTOFF, ShadowRef
from test_gpu_random import random_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a lighting, a shadow, a clip, a layout or a forced path behind"""
    yield
    gpu.clear_lighting()
    gpu.clear_shadow()
    gpu.clear_clip()
    gpu.set_layout(vr.LAYOUT_BRICKED)
    gpu.set_wide_addressing(0)
    gpu.set_tile_mapping(-1)
    gpu.set_tile_scheduling(1)
    gpu.set_brick_plane(-1)


def diff(a, b):
    return int((a != b).any(axis=-1).sum())


def depth_diff(a, b):
    return int((depth_bits(a) != depth_bits(b)).sum())


def load(gpu, scene, window):
    gpu.set_window_buffer(*window)
    gpu.set_transfer_fn(scene.tf, scene.esl)
    gpu.set_volume(scene.vox)


def set_shadow_of(gpu, f, strength=None):
    gpu.set_shadow(f.light, f.S, f.shadow_step, f.strength if strength is None else strength, CUTOFF, f.shadow_sampling)


CLEAR = ("clear_lighting", "clear_shadow", "clear_clip")


def check_frame(vr, gpu, scene, f, what):
    """The six comparisons on one frame; the context comes without a clip, a shadow and a lighting and is left so"""
    e = fr.Expected(scene, f)
    set_clip(gpu, f.clip)
    out = gpu.render_volume(f.p)
    assert diff(out, e.composite) == 0, (what, "clipped composite", diff(out, e.composite), gpu.last_launch())
    for esl in (0, 1):
        out = gpu.render_mip(fr.with_sampling(f.mip, f.mip.sampling, esl))
        assert diff(out, e.mip) == 0, (what, "mip", f.mip.sampling, esl, diff(out, e.mip))
        out, depth = gpu.render_iso(fr.with_sampling(f.iso, f.iso.sampling, esl), f.level, f.refine, depth=True)
        assert diff(out, e.iso) == 0 and depth_diff(depth, e.depth) == 0, (what, "iso", f.iso.sampling, esl, f.level, f.refine, diff(out, e.iso), depth_diff(depth, e.depth))
    set_shadow_of(gpu, f)
    q = gpu.download_shadow()
    assert q.shape == e.q.shape and np.array_equal(q, e.q), (what, "light grid", f.light, f.S, f.shadow_step, f.shadow_sampling, int((q != e.q).sum()))
    out = gpu.render_volume(f.p)
    info = gpu.last_launch()
    assert diff(out, e.shadowed) == 0, (what, "shadowed", f.light, f.S, f.strength, diff(out, e.shadowed), info)
    assert info["shadowed"] == 1 and info["layout"] in (0, 1, 5), (what, info)
    gpu.set_lighting(*f.lighting)
    before = gpu.lighting_frames()
    out = gpu.render_volume(f.p)
    info = gpu.last_launch()
    assert diff(out, e.lit) == 0, (what, "lit", f.lighting, diff(out, e.lit), info)
    assert info["layout"] in (0, 1, 5) and info["shadowed"] == 1 and gpu.lighting_frames() == before + 1, (what, info)
    for i in f.clear_order:
        getattr(gpu, CLEAR[i])()
    return e


def test_random_scenes_match_the_restatements(vr, gpu, oracle):
    """14 random scenes x 4 frames, layout and wide addressing alternating per scene.  Per frame a fresh view, clip, light, S, strength,
    lighting, level and refine: the clipped composite, the clipped MIP and isosurface with esl 0 and 1 (RGBA and depth bits), the light
    grid, the shadowed frame and the lit, shadowed, clipped frame equal the restatements; the three states are cleared in a random order and
    every second frame the plain frame is the oracle's again."""
    frames = inside = axis = nonempty = 0
    for scene in fr.random_scenes(oracle, vr):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene, (70, 50))
        for i, f in enumerate(scene.frames):
            what = (scene.describe(), "layout", scene.layout, "wide", scene.wide, "frame", i, "persp", f.p.view.perspective)
            e = check_frame(vr, gpu, scene, f, what)
            if i % 2:
                out = gpu.render_volume(f.p)
                want = oracle.render(f.p, scene.vox, scene.tf, scene.esl, threads=4)
                assert diff(out, want) == 0 and gpu.last_launch()["shadowed"] == 0, (what, "a state leaked", diff(out, want), gpu.last_launch())
            frames += 1
            inside += int(f.camera_inside())
            axis += int(f.axis_aligned())
            nonempty += int(e.lit.any())
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE
    assert inside >= 4 and axis >= 4, (inside, axis)
    assert 2 * nonempty >= frames, nonempty                # (tests/test_feature_random_model.py holds every family to this)


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
@pytest.mark.parametrize("shape", fr.EDGE_SHAPES, ids=lambda s: "x".join(str(n) for n in s))
def test_edge_shapes_match_the_restatements(vr, gpu, oracle, shape, dtype):
    """Extents of 1 and 2, one brick exactly, one voxel more than a brick, long thin volumes: benchmark views 0, 1 and 5 at 48 x 40 under BOTH
    and the identity clip, the inside light with S = 5, PHONG, level 128 — the same six comparisons, in both layouts"""
    scene = fr.edge_scene(oracle, vr, shape, dtype)
    for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
        gpu.set_layout(layout)
        load(gpu, scene, fr.EDGE_SIZE)
        for f in scene.frames:
            check_frame(vr, gpu, scene, f, (shape, dtype, "layout", layout, "view", f.view, f.clip_name))
    assert len(scene.frames) == 6


def test_state_changes_between_frames_rebuild_the_grid(vr, gpu, oracle):
    """24 random operations on one context — another volume, another transfer function, a clip, no clip, a shadow (changed, the same again,
    the strength alone), a lighting — each followed by a download: the grid is the restatement's for the state as it stands, and it was
    built again exactly when something it depends on changed"""
    rng = fr.generator(1)
    ref = ShadowRef.instance()
    scenes = [random_scene(rng, oracle, vr) for _ in range(3)]
    state = {"vox": scenes[0][0], "tf": scenes[0][1], "clip": None}
    gpu.set_window_buffer(70, 50)
    gpu.set_transfer_fn(state["tf"], scenes[0][2])
    gpu.set_volume(state["vox"])

    def new_shadow():
        S = int(rng.choice(fr.SHADOW_DIMS))
        return {"light": fr.random_light(rng, S), "S": S, "step": fr.clamp_step(rng.uniform(0.03, 0.3)), "sampling": int(rng.choice([1, 2]))}
    shadow, strength = new_shadow(), 1.0
    gpu.set_shadow(shadow["light"], shadow["S"], shadow["step"], strength, CUTOFF, shadow["sampling"])
    gpu.download_shadow()
    builds = gpu.shadow_builds()[0]
    rebuilt = kept = 0
    done = set()
    for n in range(24):
        op = ("set_volume", "set_transfer_fn", "set_clip", "clear_clip", "set_shadow", "same_shadow", "strength", "set_lighting")[n if n < 8 else int(rng.integers(0, 8))]
        changed = True
        if op == "set_volume":
            vox = scenes[int(rng.integers(0, 3))][0]
            vox = vox[::-1].copy() if vox is state["vox"] else vox                       # always another volume
            state["vox"] = vox
            gpu.set_volume(vox)
        elif op == "set_transfer_fn":
            base = rng.random((128, 4)).astype(np.float32)
            base[: int(rng.integers(0, 40)), 3] = 0
            tf, esl = oracle.update_transfer_fn(base, oracle.volume_minmax(state["vox"])[0])
            state["tf"] = tf
            gpu.set_transfer_fn(tf, esl)
        elif op == "set_clip":
            state["clip"] = fr.random_clip(rng)
            set_clip(gpu, state["clip"])
        elif op == "clear_clip":
            changed = state["clip"] is not None
            state["clip"] = None
            gpu.clear_clip()
        elif op == "set_shadow":
            shadow = new_shadow()
            gpu.set_shadow(shadow["light"], shadow["S"], shadow["step"], strength, CUTOFF, shadow["sampling"])
        elif op == "same_shadow":
            changed = False
            gpu.set_shadow(shadow["light"], shadow["S"], shadow["step"], strength, CUTOFF, shadow["sampling"])
        elif op == "strength":
            changed = False
            strength = float(np.float32(rng.uniform(0.0, 1.0)))
            gpu.set_shadow(shadow["light"], shadow["S"], shadow["step"], strength, CUTOFF, shadow["sampling"])
        else:
            changed = False
            gpu.set_lighting(*fr.random_lighting(rng))
        q = gpu.download_shadow()
        want = ref.build(shadow["light"], shadow["S"], shadow["step"], state["vox"], state["tf"], CUTOFF, shadow["sampling"], clip=state["clip"])
        assert np.array_equal(q, want), (n, op, shadow, state["clip"], int((q != want).sum()))
        builds += int(changed)
        assert gpu.shadow_builds()[0] == builds, (n, op, changed, gpu.shadow_builds()[0], builds)
        rebuilt += int(changed)
        kept += int(not changed)
        done.add(op)
    assert len(done) == 8 and rebuilt >= 5 and kept >= 4, (done, rebuilt, kept)


def _rows_of(rank, world, band_rows, out_rows):
    return [((ly // band_rows) * world + rank) * band_rows + ly % band_rows for ly in range(out_rows)]


def test_random_frames_partitioned(vr, gpu, oracle):
    """Four random lit, shadowed, clipped frames, one MIP and one isosurface frame: every rank of an interleaved band partition (2 or 3
    ranks, bands of 1, 3 or 16 rows) holds the matching rows of the whole frame and zeros (depth -1) past its end, and a crop in x its columns"""
    rng = fr.generator(2)
    scenes = fr.random_scenes(oracle, vr, stream=3, scenes=4, frames=1)
    checked = 0
    for n, scene in enumerate(scenes):
        f = scene.frames[0]
        for _ in range(20):                                  # a frame tall and wide enough to be split, with something in it
            e = fr.Expected(scene, f)
            if f.p.view.height >= 8 and f.p.view.width >= 8 and e.lit.any():
                break
            f = fr.random_frame(rng, vr, scene)
        assert f.p.view.height >= 8 and e.lit.any(), n
        load(gpu, scene, (70, 50))
        set_clip(gpu, f.clip)
        w, h = f.p.view.width, f.p.view.height
        kinds = [("lit", f.p, e.lit, None)]
        if n == 0:
            kinds.append(("mip", fr.with_sampling(f.mip, f.mip.sampling, 1), e.mip, None))
        if n == 1:
            kinds.append(("iso", fr.with_sampling(f.iso, f.iso.sampling, 1), e.iso, e.depth))
        for kind, whole, want, want_depth in kinds:
            if kind == "lit":
                set_shadow_of(gpu, f)
                gpu.set_lighting(*f.lighting)
            else:
                gpu.clear_shadow()
                gpu.clear_lighting()

            def render(p):
                if kind == "lit":
                    return gpu.render_volume(p), None
                if kind == "mip":
                    return gpu.render_mip(p), None
                return gpu.render_iso(p, f.level, f.refine, depth=True)
            world, band_rows = int(rng.choice([2, 3])), int(rng.choice([1, 3, 16]))
            for rank in range(world):
                p, per_rank = vr.band_partition(whole.copy(), rank, world, band_rows)
                out, depth = render(p)
                assert out.shape == (per_rank * band_rows, w, 4)
                for ly, gy in enumerate(_rows_of(rank, world, band_rows, out.shape[0])):
                    assert np.array_equal(out[ly], want[gy] if gy < h else np.zeros_like(want[0])), (n, kind, world, band_rows, rank, ly, gy)
                    if depth is not None:
                        assert np.array_equal(depth_bits(depth[ly]), depth_bits(want_depth[gy] if gy < h else np.full(w, -1, np.float32))), (n, kind, world, band_rows, rank, ly, gy)
                checked += 1
            x0 = int(rng.integers(0, w - 3))
            cw = int(rng.integers(1, w - x0 + 1))
            crop = whole.copy()
            crop.x0, crop.out_width = x0, cw
            out, depth = render(crop)
            assert np.array_equal(out, want[:, x0:x0 + cw]), (n, kind, "crop", x0, cw)
            if depth is not None:
                assert np.array_equal(depth_bits(depth), depth_bits(want_depth[:, x0:x0 + cw])), (n, kind, "crop depth", x0, cw)
            checked += 1
    assert checked >= 6 * 3


BOUNDS_LIB = os.path.join(ROOT, "build_variants", "libvr_hip_bounds.so")
EDGE_CASES = len(fr.EDGE_SHAPES) * len(fr.EDGE_DTYPES)


@pytest.mark.skipif(not os.path.exists(BOUNDS_LIB), reason="build_variants/libvr_hip_bounds.so not built (scripts/build_variant.sh bounds -DVR_BOUNDS_CHECK)")
def test_under_the_bounds_checked_build():
    """The random scenes and the edge shapes once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every
    gather address — the gradient fetches at the faces, the tail bricks, the padded address tables of an extent of 1 — is held against its
    array.  A violation fails the frame (VrError); nothing faults; the bytes still equal the restatements."""
    env = dict(os.environ, VR_HIP_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q",
                        "-k", "random_scenes_match or edge_shapes_match"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and f"{1 + EDGE_CASES} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
