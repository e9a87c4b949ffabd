"""Randomised and ragged-volume parity of the newer render features: the clipped composite, the MIP, the isosurface with depth, the light
grid, the shadowed and the gradient-lit frames on the random volumes and views of tests/test_gpu_random.py (odd extents, an extent of
1 / 2 / 8 / 16 / 33, cameras inside the cube, exact zeros in the direction, the four-fold ray step) under a random clip, light, grid size,
lighting and level per frame, and on the hand-made EDGE_SHAPES — every byte equal to the restatements of tests/feature_ref.c (the clip_*,
shadow_* and light_render entry points); and, on the same frames, the pre-integrated (slab) composite, the backdrop frame over a synthetic
layer and the hybrid of isosurface and volume against its slab_render, backdrop_render and hybrid_render.  tests/feature_random.py draws
the frames; tests/test_feature_random_model.py ties the restatements to one another on them
and shows that they are neither empty nor untouched by the feature.  Other seeds: VR_TEST_SEED=... pytest -m gpu tests/test_gpu_feature_random.py"""
import numpy as np
import pytest

import feature_random as fr
from clip_helpers import IDENTITY, ClipRef, set_clip
from gpu_feature import depth_diff, diff, load, needs_bounds_lib, reset_context, run_under_bounds_build
from iso_helpers import depth_bits
from light_helpers import LightRef
from shadow_helpers import CUTOFF, ShadowRef
from test_gpu_random import random_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def state_off_afterwards(vr, gpu):
    """the context is shared by the whole session: no test leaves a state, a layout or a forced path behind"""
    yield
    reset_context(vr, gpu)


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
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
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
        load(gpu, scene.vox, scene.tf, scene.esl, fr.EDGE_SIZE)
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


CLEAR_ALL = CLEAR + ("clear_preintegration",)


def all_states_on(gpu, f):
    gpu.set_preintegration()
    set_shadow_of(gpu, f)
    gpu.set_lighting(*f.lighting)


def all_states_off(gpu):
    gpu.clear_preintegration()
    gpu.clear_shadow()
    gpu.clear_lighting()


def check_layer_frame(vr, gpu, scene, f, salt, what, frame_index, in_place):
    """The slab, backdrop and hybrid comparisons on one frame under its clip; the context comes without a clip, a shadow, a lighting and
    the pre-integration and is left so, the four cleared in the frame's order with the pre-integration at position frame_index % 4"""
    e = fr.ExpectedLayers(scene, f, salt)
    set_clip(gpu, f.clip)
    gpu.set_preintegration()
    counts = gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()
    out = gpu.render_volume(f.p)
    assert diff(out, e.slab) == 0, (what, "slab", diff(out, e.slab), gpu.last_launch())
    set_shadow_of(gpu, f)
    gpu.set_lighting(*f.lighting)
    out = gpu.render_volume(f.p)
    info = gpu.last_launch()
    assert diff(out, e.slab_all) == 0, (what, "slab, lit and shadowed", f.lighting, f.light, f.S, f.strength, diff(out, e.slab_all), info)
    assert info["layout"] in (0, 1, 5) and info["shadowed"] == 1, (what, info)
    assert (gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()) == (counts[0] + 2, counts[1] + 1, counts[2]), (what, counts)
    all_states_off(gpu)
    counts = gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()
    out = gpu.render_backdrop(f.p, e.rgba, e.depth)
    info = gpu.last_launch()
    assert diff(out, e.backdrop) == 0, (what, "backdrop", diff(out, e.backdrop), info)
    assert info["ordered"] == 0 and info["layout"] in (0, 1, 5) and info["shadowed"] == 0, (what, info)
    assert (gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()) == (counts[0], counts[1], counts[2] + 1), (what, counts)
    if in_place:
        import torch
        layer = torch.from_numpy(np.array(e.rgba)).cuda()
        dlayer = torch.from_numpy(np.array(e.depth)).cuda()
        torch.cuda.synchronize()                        # (the uploads run on torch's stream, the frame on the context's)
        gpu.render_backdrop_device(f.p, layer.data_ptr(), dlayer.data_ptr(), layer.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert diff(layer.cpu().numpy(), e.backdrop) == 0, (what, "backdrop in place", diff(layer.cpu().numpy(), e.backdrop))
        assert depth_diff(dlayer.cpu().numpy(), e.depth) == 0, (what, "the depth layer of a frame in place")
    out, depth = gpu.render_hybrid(f.p, f.level, f.refine, depth=True)
    assert diff(out, e.hybrid) == 0 and depth_diff(depth, e.hybrid_depth) == 0, (what, "hybrid", f.level, f.refine, diff(out, e.hybrid), depth_diff(depth, e.hybrid_depth))
    all_states_on(gpu, f)
    counts = gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()
    out = gpu.render_backdrop(f.p, e.rgba, e.depth)
    info = gpu.last_launch()
    assert diff(out, e.backdrop_all) == 0, (what, "backdrop under all four states", diff(out, e.backdrop_all), info)
    assert info["ordered"] == 0 and info["layout"] in (0, 1, 5) and info["shadowed"] == 1, (what, info)
    out, depth = gpu.render_hybrid(f.p, f.level, f.refine, depth=True)
    assert diff(out, e.hybrid_all) == 0 and depth_diff(depth, e.hybrid_depth) == 0, (what, "hybrid under all four states", diff(out, e.hybrid_all), depth_diff(depth, e.hybrid_depth))
    assert (gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()) == (counts[0] + 2, counts[1] + 2, counts[2] + 2), (what, counts)
    out = gpu.render_iso(f.p, f.level, f.refine)
    assert diff(out, e.hybrid_iso) == 0, (what, "the isosurface ignores shadow, lighting and pre-integration", diff(out, e.hybrid_iso))
    order = [CLEAR[i] for i in f.clear_order]
    order.insert(frame_index % 4, "clear_preintegration")
    assert sorted(order) == sorted(CLEAR_ALL)
    for name in order:
        getattr(gpu, name)()
    return e


def test_random_scenes_slab_backdrop_hybrid(vr, gpu, oracle):
    """The 14 x 4 random frames once more, layout and wide addressing alternating per scene, every frame of another size (1..69 x 1..49:
    the staging and depth buffers grow and shrink) under its clip: the pre-integrated composite alone and with the frame's shadow and
    lighting; the backdrop frame over a synthetic layer (random colour words; depths -1, NaN, 0, +inf, before, inside and beyond the
    clipped segment and exactly on a sample) and the hybrid at the frame's level with its depth bits, both point classified and under all
    four states; the isosurface frame afterwards; on each scene's first frame the device entry point in place.  Every byte is the
    restatements'; the counters move as the contract says; the four states are cleared in a random order and every second frame the plain
    frame is the oracle's again."""
    frames = inside = axis = nonempty = 0
    for s, scene in enumerate(fr.random_scenes(oracle, vr)):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
        for i, f in enumerate(scene.frames):
            what = (scene.describe(), "layout", scene.layout, "wide", scene.wide, "frame", i, "persp", f.p.view.perspective, (f.p.view.width, f.p.view.height))
            e = check_layer_frame(vr, gpu, scene, f, fr.layer_salt(s, i), what, i, in_place=i == 0)
            if i % 2:
                out = gpu.render_volume(f.p)
                want = oracle.render(f.p, scene.vox, scene.tf, scene.esl, threads=4)
                assert diff(out, want) == 0 and gpu.last_launch()["shadowed"] == 0, (what, "a state leaked", diff(out, want), gpu.last_launch())
            frames += 1
            inside += int(f.camera_inside())
            axis += int(f.axis_aligned())
            nonempty += int(e.backdrop.any())
    assert frames == fr.SCENES * fr.FRAMES_PER_SCENE
    assert inside >= 4 and axis >= 4, (inside, axis)
    assert 2 * nonempty >= frames, nonempty                # (tests/test_feature_random_model.py holds the slab and backdrop frames to this)


def test_holed_scenes_slab_backdrop_hybrid(vr, gpu, oracle):
    """The same comparisons on the holed scenes of tests/feature_random.py — a slab of exact zeros through a random volume under a transfer
    function with leading zeros, frames of 16 pixels or more a side: whole waves skip their samples inside the hole unresolved, and the
    first sample behind it takes its predecessor's coordinate from the fetch slot kept for it.  (The random volumes are smooth; a skipped
    sample there is followed by a transparent one.)"""
    frames = nonempty = 0
    for s, scene in enumerate(fr.holed_scenes(oracle, vr)):
        gpu.set_layout(scene.layout)
        gpu.set_wide_addressing(scene.wide)
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
        for i, f in enumerate(scene.frames):
            what = (scene.describe(), "layout", scene.layout, "wide", scene.wide, "frame", i, "persp", f.p.view.perspective, (f.p.view.width, f.p.view.height))
            e = check_layer_frame(vr, gpu, scene, f, fr.layer_salt(200 + s, i), what, i, in_place=i == 0)
            frames += 1
            nonempty += int(e.slab.any())
    assert frames == fr.HOLED_SCENES * fr.HOLED_FRAMES and 2 * nonempty >= frames, (frames, nonempty)


@pytest.mark.parametrize("dtype", fr.EDGE_DTYPES)
@pytest.mark.parametrize("shape", fr.EDGE_SHAPES, ids=lambda s: "x".join(str(n) for n in s))
def test_edge_shapes_hybrid(vr, gpu, oracle, shape, dtype):
    """The hybrid with its depth bits on the EDGE_SHAPES, six frames each in both layouts: point classified, and under the inside light's
    grid, PHONG and the pre-integration (tests/test_gpu_slab.py and tests/test_gpu_backdrop.py hold the slab and backdrop frames of these shapes)"""
    scene = fr.edge_scene(oracle, vr, shape, dtype)
    for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
        gpu.set_layout(layout)
        load(gpu, scene.vox, scene.tf, scene.esl, fr.EDGE_SIZE)
        for f in scene.frames:
            what = (shape, dtype, "layout", layout, "view", f.view, f.clip_name)
            e = fr.ExpectedLayers(scene, f)
            set_clip(gpu, f.clip)
            all_states_off(gpu)
            out, depth = gpu.render_hybrid(f.p, f.level, f.refine, depth=True)
            assert diff(out, e.hybrid) == 0 and depth_diff(depth, e.hybrid_depth) == 0, (what, "hybrid", diff(out, e.hybrid), depth_diff(depth, e.hybrid_depth), gpu.last_launch())
            all_states_on(gpu, f)
            out, depth = gpu.render_hybrid(f.p, f.level, f.refine, depth=True)
            assert diff(out, e.hybrid_all) == 0 and depth_diff(depth, e.hybrid_depth) == 0, (what, "all four states", diff(out, e.hybrid_all), depth_diff(depth, e.hybrid_depth), gpu.last_launch())
    assert len(scene.frames) == 6


STATE_KINDS = ("volume", "transfer_fn", "clip", "preintegration", "shadow", "lighting", "backdrop", "hybrid", "composite", "mip")


def test_state_changes_between_slab_and_backdrop_frames(vr, gpu, oracle):
    """32 operations on one context at a fixed 64 x 48 view — another volume, another random transfer function, a clip set or cleared, the
    pre-integration switched, another shadow, a lighting set or cleared, a backdrop frame, a hybrid frame, a plain composite frame, a MIP;
    the first ten run each kind once — each followed by one frame of a random kind (composite, backdrop, hybrid) held against the
    restatement for the state as it stands.  After every transfer function K is slab_build_integral's of tests/feature_ref.c, bit for bit; the three frame counters
    move as the contract says; the light grid is built again exactly when something it depends on changed — never for the pre-integration,
    a lighting, or a backdrop or hybrid frame."""
    from backdrop_helpers import BackdropRef, synthetic_layer
    from slab_helpers import POINT, SLAB, SlabRef
    rng = fr.generator(4)
    ref, slab_ref, shadow_ref, clip_ref = BackdropRef.instance(), SlabRef.instance(), ShadowRef.instance(), ClipRef.instance()
    volumes = []
    for _ in range(3):
        vox, _, _, bd, bs, ray_step = random_scene(rng, oracle, vr)
        vox = np.ascontiguousarray(vox)
        vox.setflags(write=False)
        volumes.append((vox, bd, bs, fr.clamp_step(ray_step), oracle.volume_minmax(vox)[0]))
    view = vr.benchmark_view(64, 48, 5)
    st = {"volume": 0, "base": oracle.default_base_tf(), "clip": None, "preint": False, "lighting": None, "strength": 1.0}

    def params():
        vox, bd, bs, step, _ = volumes[st["volume"]]
        p = vr.VrParams()
        p.view = view
        p.ray_step, p.light_kd, p.ray_threshold, p.esl, p.esl_block_dims = step, 0.7, 0.95, 1, int(bd)
        for j in range(3):
            p.esl_block_size[j] = float(bs[j])
        p.sampling = st["sampling"]
        return vr.whole_frame(p)

    def upload_tf():
        st["tf"], st["esl"] = oracle.update_transfer_fn(st["base"], volumes[st["volume"]][4])
        gpu.set_transfer_fn(st["tf"], st["esl"])
        K = gpu.download_tf_integral()
        assert np.array_equal(K.view(np.uint32), slab_ref.integral(st["tf"]).view(np.uint32)), "the integral table after a transfer function"

    def new_shadow():
        S = int(rng.choice(fr.SHADOW_DIMS))
        st["shadow"] = {"light": fr.random_light(rng, S), "S": S, "step": fr.clamp_step(rng.uniform(0.03, 0.3)), "sampling": int(rng.choice([1, 2]))}
        st["strength"] = float(np.float32(rng.uniform(0.2, 1.0)))
        gpu.set_shadow(st["shadow"]["light"], S, st["shadow"]["step"], st["strength"], CUTOFF, st["shadow"]["sampling"])

    def frame(kind, salt):
        """one frame of `kind` under the state as it stands, held against its restatement; the counters move as the contract says"""
        vox = volumes[st["volume"]][0]
        tf, esl, p = st["tf"], st["esl"], params()
        clip = st["clip"] if st["clip"] is not None else IDENTITY
        sh = st["shadow"]
        counts = gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()
        if kind == "mip":
            out = gpu.render_mip(p)
            want = clip_ref.mip(fr.with_sampling(p, p.sampling, 0), vox, tf, clip)
            assert diff(out, want) == 0, (kind, diff(out, want))
            assert (gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()) == counts
            return want
        q = shadow_ref.build(sh["light"], sh["S"], sh["step"], vox, tf, CUTOFF, sh["sampling"], clip=st["clip"])
        states = (SLAB if st["preint"] else POINT, clip, st["lighting"], q, st["strength"])
        if kind == "composite":
            out = gpu.render_volume(p)
            want = slab_ref.render(p, vox, tf, esl, *states)
        elif kind == "backdrop":
            rgba, depth = synthetic_layer(ref, p, vox, tf, esl, clip, salt=salt)
            out = gpu.render_backdrop(p, rgba, depth)
            want = ref.render(p, vox, tf, esl, rgba, depth, *states)
        else:
            level, refine = fr.random_level(rng, vox, tf), int(rng.integers(0, 9))
            out, depth = gpu.render_hybrid(p, level, refine, depth=True)
            want, want_depth, _ = ref.hybrid(p, vox, tf, esl, level, refine, *states)
            assert depth_diff(depth, want_depth) == 0, (kind, level, refine, depth_diff(depth, want_depth))
        info = gpu.last_launch()
        assert diff(out, want) == 0, (kind, st["preint"], st["lighting"], st["clip"], sh, st["strength"], diff(out, want), info)
        assert info["shadowed"] == 1, info
        moved = (counts[0] + int(st["preint"]), counts[1] + int(st["lighting"] is not None), counts[2] + int(kind != "composite"))
        assert (gpu.preint_frames(), gpu.lighting_frames(), gpu.backdrop_frames()) == moved, (kind, counts, moved)
        return want

    gpu.set_window_buffer(70, 50)
    st["sampling"] = int(rng.choice([vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8]))
    upload_tf()
    gpu.set_volume(volumes[0][0])
    new_shadow()
    frame("composite", 0)
    builds = gpu.shadow_builds()[0]
    done, rebuilt, kept, nonempty = set(), 0, 0, 0
    for n in range(32):
        op = STATE_KINDS[n if n < len(STATE_KINDS) else int(rng.integers(0, len(STATE_KINDS)))]
        stale = False                                    # does the light grid depend on what this operation changes?
        if op == "volume":
            st["volume"] = (st["volume"] + int(rng.integers(1, 3))) % 3                    # always another volume
            gpu.set_volume(volumes[st["volume"]][0])
            upload_tf()                                  # the empty-block bits are the new volume's
            st["sampling"] = int(rng.choice([vr.SAMPLE_TRILINEAR, vr.SAMPLE_TRILINEAR_Q8]))
            stale = True
        elif op == "transfer_fn":
            base = rng.random((128, 4)).astype(np.float32)
            base[:, 3] *= (rng.random(128) < 0.7)
            base[: int(rng.integers(0, 40)), 3] = 0
            st["base"] = base
            upload_tf()
            stale = True
        elif op == "clip":
            if st["clip"] is not None and rng.random() < 0.5:
                st["clip"] = None
                gpu.clear_clip()
            else:
                st["clip"] = fr.random_clip(rng)
                set_clip(gpu, st["clip"])
            stale = True
        elif op == "preintegration":
            st["preint"] = not st["preint"]
            gpu.set_preintegration(st["preint"])
        elif op == "shadow":
            new_shadow()
            stale = True
        elif op == "lighting":
            if st["lighting"] is not None and rng.random() < 0.5:
                st["lighting"] = None
                gpu.clear_lighting()
            else:
                st["lighting"] = fr.random_lighting(rng)
                gpu.set_lighting(*st["lighting"])
        else:
            frame(op, 3500 + 2 * n)
        kind = ("composite", "backdrop", "hybrid")[int(rng.integers(0, 3))]
        nonempty += int(frame(kind, 3501 + 2 * n).any())
        builds += int(stale)
        assert gpu.shadow_builds()[0] == builds, (n, op, kind, stale, gpu.shadow_builds()[0], builds)
        rebuilt, kept = rebuilt + int(stale), kept + int(not stale)
        done.add(op)
    assert done == set(STATE_KINDS) and rebuilt >= 4 and kept >= 6 and 2 * nonempty >= 32, (done, rebuilt, kept, nonempty)


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
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
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


def test_random_slab_and_hybrid_frames_partitioned(vr, gpu, oracle):
    """Four more random frames: the pre-integrated, lit, shadowed, clipped composite, the backdrop frame and the hybrid with its depth.
    Every rank of an interleaved band partition (2 or 3 ranks, bands of 1, 3 or 16 rows) holds the matching rows of the whole frame and a
    crop in x its columns.  The layers of the backdrop are partitioned like the output, with depth -1 in the rows past the view's end,
    which are zeros then; the hybrid's isosurface pass writes depth -1 there itself, and its composite pass reads that as no surface."""
    rng = fr.generator(6)
    scenes = fr.random_scenes(oracle, vr, stream=5, scenes=4, frames=1)
    checked = 0
    for n, scene in enumerate(scenes):
        f = scene.frames[0]
        for _ in range(20):                                  # a frame tall and wide enough to be split, with something in it
            e = fr.ExpectedLayers(scene, f, fr.layer_salt(100 + n, 0))
            if f.p.view.height >= 8 and f.p.view.width >= 8 and e.slab_all.any():
                break
            f = fr.random_frame(rng, vr, scene)
        assert f.p.view.height >= 8 and f.p.view.width >= 8 and e.slab_all.any(), n
        load(gpu, scene.vox, scene.tf, scene.esl, (70, 50))
        set_clip(gpu, f.clip)
        w, h = f.p.view.width, f.p.view.height
        nothing, no_depth = np.zeros((w, 4), np.uint8), np.full(w, -1, np.float32)
        for kind, want, want_depth in (("slab", e.slab_all, None), ("backdrop", e.backdrop, None), ("hybrid", e.hybrid, e.hybrid_depth)):
            if kind == "slab":
                all_states_on(gpu, f)
            else:
                all_states_off(gpu)

            def render(p, rows, cols):
                """the frame of `p`, whose output rows are the whole frame's `rows` (-1: past the view's end) and columns `cols`"""
                if kind == "slab":
                    return gpu.render_volume(p), None
                if kind == "hybrid":
                    return gpu.render_hybrid(p, f.level, f.refine, depth=True)
                rgba = rng.integers(0, 256, size=(len(rows), cols.stop - cols.start, 4), dtype=np.uint8)
                depth = np.full(rgba.shape[:2], -1, np.float32)
                for ly, gy in enumerate(rows):
                    if gy >= 0:
                        rgba[ly], depth[ly] = e.rgba[gy, cols], e.depth[gy, cols]
                return gpu.render_backdrop(p, rgba, depth), None
            world, band_rows = int(rng.choice([2, 3])), int(rng.choice([1, 3, 16]))
            for rank in range(world):
                p, per_rank = vr.band_partition(f.p.copy(), rank, world, band_rows)
                rows = [gy if gy < h else -1 for gy in _rows_of(rank, world, band_rows, per_rank * band_rows)]
                out, depth = render(p, rows, slice(0, w))
                assert out.shape == (per_rank * band_rows, w, 4)
                for ly, gy in enumerate(rows):
                    assert np.array_equal(out[ly], want[gy] if gy >= 0 else nothing), (n, kind, world, band_rows, rank, ly, gy)
                    if depth is not None:
                        assert np.array_equal(depth_bits(depth[ly]), depth_bits(want_depth[gy] if gy >= 0 else no_depth)), (n, kind, world, band_rows, rank, ly, gy)
                checked += 1
            x0 = int(rng.integers(0, w - 3))
            cw = int(rng.integers(1, w - x0 + 1))
            crop = f.p.copy()
            crop.x0, crop.out_width = x0, cw
            out, depth = render(crop, list(range(h)), slice(x0, x0 + cw))
            assert np.array_equal(out, want[:, x0:x0 + cw]), (n, kind, "crop", x0, cw)
            if depth is not None:
                assert np.array_equal(depth_bits(depth), depth_bits(want_depth[:, x0:x0 + cw])), (n, kind, "crop depth", x0, cw)
            checked += 1
    assert checked >= 4 * 3 * 3


EDGE_CASES = len(fr.EDGE_SHAPES) * len(fr.EDGE_DTYPES)


@needs_bounds_lib
def test_under_the_bounds_checked_build():
    """The random scenes and the edge shapes (the slab, backdrop and hybrid frames among them) once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py): every
    gather address — the gradient fetches at the faces, the tail bricks, the padded address tables of an extent of 1 — is held against its
    array.  A violation fails the frame (VrError); nothing faults; the bytes still equal the restatements."""
    run_under_bounds_build(__file__, "random_scenes_match or edge_shapes_match or random_scenes_slab or holed_scenes or edge_shapes_hybrid", 3 + 2 * EDGE_CASES,
                           timeout=1200)
