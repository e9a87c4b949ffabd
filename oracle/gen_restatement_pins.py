#!/usr/bin/env python3
"""Hashes of what the CPU restatements of tests/ (the seven *Ref classes of tests/*_helpers.py) return: tests/golden/restatement_pins.json.
TEST INFRASTRUCTURE.

The restatements are what every GPU parity test compares with, so a change to their text must change none of their outputs.  This script
calls only the public methods of MipRef, IsoRef, ClipRef, ShadowRef, LightRef, SlabRef and BackdropRef and takes helpers.fnv1a32 of
every array they return (frame bytes, depth bits, light grids, integral tables, segments) and their counters as integers, so it runs
unchanged on any arrangement of the C text behind those classes.  To keep the fixture small, an entry (one entry point on one case, all
its argument variants and clips) keeps one fnv1a32 over those hashes and counters (fold() below).  tests/test_restatement_pins.py walks
the same list (pins() below) and asserts every recorded value.  The committed fixture was taken at the commit named in it; regenerate it only when a restatement is MEANT
to compute something else.

What is walked:
  golden/...   every golden case with a frame but the sixteen 256 x 256 benchmark frames — the largest cases, which would treble the test's
               time; the 64 x 64 frames of the same eight views are among the rest and the *_model.py ties still walk them —, TRILINEAR and Q8 (NEAREST too for clip_render), under the identity clip and each of clip_helpers.CLIPS: the clipped
               composite with and without the cue; the shadowed frame without a grid, with any grid at strength 0 and with a built grid at
               strength 0, 0.6 and 1; the lit frame under the identity lighting and PHONG, with and without the grid; slab modes 0-3 under the
               cue and under PHONG with the grid; the backdrop frame without layers, and perturb 0-3 over a synthetic layer; the segments;
               the hybrid at backdrop_helpers.HYBRID_LEVELS.  The MIP and the isosurface on the small cases tests/test_clip_model.py uses.
  random/..., holed/..., edge/...   the frames of tests/feature_random.py, every restatement called as Expected / ExpectedLayers and the
               tie tests of tests/test_feature_random_model.py call it.
  the light grids of shadow_helpers.GRID_SCENES with a clip and without, the isosurface of iso_helpers.PAIRS with and without the
  skipping emulation, the integral tables of slab_helpers.peak_tf / holed_tf.

usage: gen_restatement_pins.py      (from a tree whose library and oracle are built)
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, "tests", "golden", "restatement_pins.json")

GRID_S, STRENGTH = 9, 0.6                   # the light grid and the mid strength of the ties of tests/test_slab_model.py
SMALL_CASES = (32, 34, 36, 38, 40, 45)      # the golden cases of tests/test_mip_model.py: no ESL, at most 120 x 96 pixels
ISO_LEVELS, REFINE = (30.5, 100.0, 200.0), 4
LAYER_SALT = 1000                           # synthetic layers of the golden cases: LAYER_SALT + case id (the tests stay below, the random frames above)
PAIR_VIEWS = ("view1", "view5", "far_persp")


def digest(value):
    """fnv1a32 of an array's bytes (floats by their bits), an integer as it is, a tuple or dict element by element"""
    from helpers import fnv1a32
    if isinstance(value, dict):
        return {k: digest(v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return [digest(v) for v in value]
    if isinstance(value, np.ndarray):
        return fnv1a32(value)
    return int(value)


def fold(digested):
    """What the fixture keeps of one entry: fnv1a32 over the hashes of its arrays and its counters (as decimal text), in order.  Every byte
    of every output and every counter is under that one hash; which of them moved is found by printing digest() on the two trees."""
    from helpers import fnv1a32
    leaves = []

    def walk(v):
        if isinstance(v, (dict, list)):
            for x in (v.values() if isinstance(v, dict) else v):
                walk(x)
        else:
            leaves.append(str(v))
    walk(digested)
    return fnv1a32(np.frombuffer(" ".join(leaves).encode(), np.uint8))


def golden_pins(vr, golden):
    from backdrop_helpers import HYBRID_LEVELS, BackdropRef, synthetic_layer
    from clip_helpers import CLIPS, IDENTITY, ClipRef
    from iso_helpers import IsoRef
    from light_helpers import IDENTITY_LIGHTING, PHONG, LightRef, cue
    from mip_helpers import MipRef, ramp_tf
    from shadow_helpers import LIGHTS, ShadowRef
    from slab_helpers import POINT, SLAB, SlabRef
    clip_ref, shadow_ref, light_ref, slab_ref, ref = ClipRef.instance(), ShadowRef.instance(), LightRef.instance(), SlabRef.instance(), BackdropRef.instance()
    clips = (("identity", IDENTITY),) + tuple(sorted(CLIPS.items()))
    any_grid = np.random.default_rng(3).integers(0, 256, size=(5, 5, 5), dtype=np.uint8)

    def one_clip(case, p, vox, tf, esl, clip, level):
        yield "clip_render", {"cue": clip_ref.composite(p, vox, tf, esl, clip), "unlit": clip_ref.composite(cue(p), vox, tf, esl, clip)}
        if p.sampling == 0:
            return
        q = shadow_ref.build(LIGHTS["top"], GRID_S, p.ray_step, vox, tf)
        lit = (PHONG, q, STRENGTH)
        yield "shadow_build", {"q": q}
        yield "shadow_render", {"no grid": shadow_ref.render(p, vox, tf, esl, None, 1.0, clip),
                                "any grid at 0": shadow_ref.render(p, vox, tf, esl, any_grid, 0.0, clip),
                                **{f"strength {s}": shadow_ref.render(p, vox, tf, esl, q, s, clip) for s in (0.0, STRENGTH, 1.0)}}
        yield "light_render", {"identity": light_ref.render(p, vox, tf, esl, IDENTITY_LIGHTING, clip=clip, counters=True),
                               "phong": light_ref.render(p, vox, tf, esl, PHONG, clip=clip, counters=True),
                               "phong, grid": light_ref.render(p, vox, tf, esl, PHONG, q, STRENGTH, clip=clip, counters=True)}
        out = {"mode 0, grid": slab_ref.render(p, vox, tf, esl, POINT, clip, q=q, strength=STRENGTH),
               "mode 0, phong": slab_ref.render(p, vox, tf, esl, POINT, clip, PHONG)}
        for mode in (0, 1, 2, 3):
            out[f"mode {mode}"] = slab_ref.render(p, vox, tf, esl, mode, clip, counters=True)
            out[f"mode {mode}, phong, grid"] = slab_ref.render(p, vox, tf, esl, mode, clip, *lit, counters=True)
        yield "slab_render", out
        rgba, depth = synthetic_layer(ref, p, vox, tf, esl, clip, salt=LAYER_SALT + case["id"])
        out = {"layer depth": depth}
        for mode in (POINT, SLAB):
            out[f"no layer, mode {mode}"] = ref.render(p, vox, tf, esl, None, None, mode, clip)
            out[f"no layer, mode {mode}, phong, grid"] = ref.render(p, vox, tf, esl, None, None, mode, clip, *lit)
        out["layer, mode 1, phong, grid"] = ref.render(p, vox, tf, esl, rgba, depth, SLAB, clip, *lit)
        for perturb in (0, 1, 2, 3):
            out[f"layer, perturb {perturb}"] = ref.render(p, vox, tf, esl, rgba, depth, POINT, clip, perturb=perturb)
        yield "backdrop_render", out
        yield "backdrop_segments", {"segments": ref.segments(p, vox, tf, esl, clip)}
        yield "hybrid_render", {"point": ref.hybrid(p, vox, tf, esl, level, REFINE, POINT, clip),
                                "mode 1, phong, grid": ref.hybrid(p, vox, tf, esl, level, REFINE, SLAB, clip, *lit)}

    for case in golden.cases(True):
        if case["label"].startswith("bench256"):
            continue
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        st = golden.volume_state(case["volume"])
        tf, esl = st["tf"], st["esl"]
        level = HYBRID_LEVELS.get(case["volume"], 100.5)
        for sampling in (0, 1, 2):
            p = golden.params(case, sampling)
            merged = {}                             # entry point -> {clip: outputs}: one entry per (case, sampling), the clips among its variants
            for clip_name, clip in clips:
                for entry, out in one_clip(case, p, vox, tf, esl, clip, level):
                    merged.setdefault(entry, {})[clip_name] = out
            for entry, out in merged.items():
                yield entry, f"golden/{case['label']}/{case['volume']}/sampling{sampling}", out
    tf = ramp_tf()
    for case in (c for c in golden.cases() if c["id"] in SMALL_CASES):
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        scale = 1.0 if vox.dtype.itemsize == 1 else 257.0
        for sampling in (0, 1, 2):
            p = golden.params(case, sampling)
            p.esl, p.ray_threshold = 0, 1.0
            cid = f"golden/{case['label']}/{case['volume']}/sampling{sampling}"
            yield "mip_render", cid, {"frame, maximum": MipRef.instance().render(p, vox, tf)}
            yield "clip_mip_render", cid, {name: clip_ref.mip(p, vox, tf, clip) for name, clip in clips}
            if sampling == 0:
                continue
            surfaces = [(lv, refine) for lv in ISO_LEVELS for refine in (0, REFINE)]
            yield "iso_render", cid, {f"level {lv}, refine {refine}": {"plain": IsoRef.instance().render(p, vox, tf, lv * scale, refine),
                                                                       "skipping": IsoRef.instance().render(p, vox, tf, lv * scale, refine, skipping=True)}
                                      for lv, refine in surfaces}
            yield "clip_iso_render", cid, {f"level {lv}, refine {refine}": {name: clip_ref.iso(p, vox, tf, lv * scale, refine, clip) for name, clip in clips}
                                           for lv, refine in surfaces}


def frame_pins(vr, oracle, scene, f, salt):
    """every restatement on one frame of tests/feature_random.py"""
    import feature_random as fr
    from clip_helpers import IDENTITY, ClipRef
    from iso_helpers import IsoRef
    from light_helpers import IDENTITY_LIGHTING, LightRef, cue
    from mip_helpers import MipRef
    from shadow_helpers import ShadowRef
    from slab_helpers import POINT, SLAB_DOUBLE, SLAB_SKIPPED_IS_NONE, SlabRef
    v, tf, esl = scene.vox, scene.tf, scene.esl
    e, layers = fr.Expected(scene, f), fr.ExpectedLayers(scene, f, salt)
    out = {"e." + k: x for k, x in sorted(vars(e).items())}                                    # Expected.composite is "e.composite"
    out.update(("l." + k, x) for k, x in sorted(vars(layers).items()) if k != "rgba")         # ExpectedLayers.slab is "l.slab"
    out["mip_render"] = MipRef.instance().render(f.mip, v, tf)
    out["iso_render"] = IsoRef.instance().render(f.iso, v, tf, f.level, f.refine)
    out["iso_render, skipping"] = IsoRef.instance().render(f.iso, v, tf, f.level, f.refine, skipping=True)
    out["clip_mip_render, identity"] = ClipRef.instance().mip(f.mip, v, tf, IDENTITY)
    out["clip_iso_render, identity"] = ClipRef.instance().iso(f.iso, v, tf, f.level, f.refine, IDENTITY)
    out["clip_iso_render, composite params"] = ClipRef.instance().iso(f.p, v, tf, f.level, f.refine, f.clip)
    for name, clip in (("identity", IDENTITY), ("clip", f.clip)):
        out[f"clip_render, {name}"] = ClipRef.instance().composite(f.p, v, tf, esl, clip)
        out[f"clip_render, unlit, {name}"] = ClipRef.instance().composite(cue(f.p), v, tf, esl, clip)
        out[f"shadow_render, no grid, {name}"] = ShadowRef.instance().render(f.p, v, tf, esl, None, 1.0, clip)
        out[f"light_render, identity lighting, {name}"] = LightRef.instance().render(f.p, v, tf, esl, IDENTITY_LIGHTING, clip=clip)
    for mode in (POINT, SLAB_DOUBLE, SLAB_SKIPPED_IS_NONE):
        out[f"slab_render, mode {mode}"] = SlabRef.instance().render(f.p, v, tf, esl, mode, f.clip, counters=True)
    return out


def feature_random_pins(vr, oracle):
    import feature_random as fr
    for s, scene in enumerate(fr.random_scenes(oracle, vr)):
        for i, f in enumerate(scene.frames):
            yield "feature_random", f"random/scene{s}/frame{i}", frame_pins(vr, oracle, scene, f, fr.layer_salt(s, i))
    for s, scene in enumerate(fr.holed_scenes(oracle, vr)):
        for i, f in enumerate(scene.frames):
            yield "feature_random", f"holed/scene{s}/frame{i}", frame_pins(vr, oracle, scene, f, fr.layer_salt(200 + s, i))
    edges = [(shape, dtype) for shape in fr.EDGE_SHAPES for dtype in fr.EDGE_DTYPES]
    for n, (shape, dtype) in enumerate(edges):
        scene = fr.edge_scene(oracle, vr, shape, dtype)
        for i, f in enumerate(scene.frames):
            yield "feature_random", f"edge/{'x'.join(map(str, shape))}/{dtype}/view{f.view}/{f.clip_name}", frame_pins(vr, oracle, scene, f, fr.EDGE_SALT + 8 * n + i)


def remaining_pins(vr, golden, oracle):
    from clip_helpers import BOTH, composite_params
    from iso_helpers import PAIRS, IsoRef, all_volumes, frame_params, views_for
    from mip_helpers import ramp_tf
    from shadow_helpers import GRID_SCENES, LIGHTS, SMALLEST, ShadowRef
    from slab_helpers import SlabRef, holed_tf, peak_tf
    volumes = all_volumes(golden)
    for name, light, S in GRID_SCENES + (SMALLEST,):
        vox = volumes[name]
        p, tf, _ = composite_params(vr, golden, oracle, name, vox, vr.benchmark_view(80, 80, 0), 1, False)
        for sampling in (1, 2):
            yield "shadow_build", f"grid/{name}/{light}/S{S}/sampling{sampling}", {
                "no clip": ShadowRef.instance().build(LIGHTS[light], S, float(p.ray_step), vox, tf, sampling=sampling),
                "both": ShadowRef.instance().build(LIGHTS[light], S, float(p.ray_step), vox, tf, sampling=sampling, clip=BOTH)}
    tf = ramp_tf()
    for name, level in PAIRS:
        vox = volumes[name]
        for label, view in views_for(vr, golden, name):
            if label not in PAIR_VIEWS:
                continue
            for sampling in (1, 2):
                p = frame_params(vr, oracle, vox, view, sampling, 0)
                yield "iso_render", f"pair/{name}/level{level}/{label}/sampling{sampling}", {
                    "plain": IsoRef.instance().render(p, vox, tf, level, REFINE), "skipping": IsoRef.instance().render(p, vox, tf, level, REFINE, skipping=True)}
    yield "slab_build_integral", "peak_tf", {"K": SlabRef.instance().integral(peak_tf())}
    yield "slab_build_integral", "holed_tf", {"K": SlabRef.instance().integral(holed_tf())}


def pins(vr, golden, oracle):
    """(entry point, case id, {what: arrays and counters}) of everything pinned, in the fixture's order"""
    yield from golden_pins(vr, golden)
    yield from feature_random_pins(vr, oracle)
    yield from remaining_pins(vr, golden, oracle)


def main():
    from helpers import Golden, Oracle
    vr = importlib.import_module("volume-rendering_amd")
    cases = {}
    for entry, cid, out in pins(vr, Golden(), Oracle()):
        assert entry not in cases.setdefault(cid, {}), (entry, cid)
        cases[cid][entry] = fold(digest(out))
    groups = {}                                     # one line of the file per golden case, scene, shape or volume
    for cid, by_entry in cases.items():
        groups.setdefault("/".join(cid.split("/")[:2]), {})[cid] = by_entry
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    with open(OUT, "w") as f:
        f.write('{"generator": "oracle/gen_restatement_pins.py", "commit": "%s", "seed": %d, "pins": [\n' % (commit, importlib.import_module("feature_random").SEED))
        f.write(",\n".join(json.dumps(g, separators=(",", ":")) for g in groups.values()))
        f.write("\n]}\n")
    print(f"wrote {OUT}: {sum(len(e) for e in cases.values())} entries of {len(cases)} cases, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
