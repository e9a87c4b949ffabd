"""Backdrop and hybrid frames on one GPU: what the layer costs per frame and what the depth limit saves.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), full-march TRILINEAR composite, same build, same
process:
  * a backdrop frame whose layer lies behind everything (d = +inf in every pixel: nothing is narrowed, every pixel reads its two layer
    elements and blends) against the identity-clipped point-classified frame, its nearest twin — the same copies, the same march,
    clip_segment included; the base family marches one sample of prefetch shallower than that twin, as raymarch_shadowed does;
  * the same for the lit, the slab and the lit slab family against the frame of that state without a layer;
  * the hybrid (one vr_hip_render_hybrid_device: the isosurface frame, then the backdrop frame in place) against the sum of an isosurface
    frame and a composite frame of the same view, at a level whose surface lies inside the shell: the difference is what the depth limit
    saves.
Kernel ms per view from vr_hip_timing (hipEvents around every launch; a hybrid is two launches).  One JSON object on stdout; nothing here
touches oracle/.

    python scripts/backdrop_probe.py [--n 1024] [--size 2048] [--reps 5] [--level 140.5]
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHONG = (0.25, 0.65, 0.4, 4)


def time_views(r, render, params, sync, warm, reps):
    """mean kernel ms per call of render(p), per view (a call may be several launches)"""
    per_view, layouts = [], []
    for p in params:
        for _ in range(warm):
            render(p)
        sync()
        r.timing_reset()
        for _ in range(reps):
            render(p)
        sync()
        per_view.append(round(r.timing().kernel_ms_sum / reps, 4))
        layouts.append(r.last_launch()["layout"])
    return per_view, layouts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=float, default=140.5, help="isosurface level of the hybrid in raw voxel units: the shell's density rises from 0 at its outer "
                    "edge to 255 in its middle (plus 0..15 of noise everywhere), so 140.5 lies inside its outer flank, behind translucent matter")
    a = ap.parse_args()
    import torch
    vr = importlib.import_module("volume-rendering_amd")
    r = vr.HipRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=r.volume_minmax()[0])
    r.set_transfer_fn(scene.tf, scene.esl)
    level = a.level
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    dbuf = torch.empty((a.size, a.size), dtype=torch.float32, device="cuda:0")
    layer = torch.randint(0, 256, (a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    far = torch.full((a.size, a.size), float("inf"), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "device": r.device_info()[0], "lighting": list(PHONG), "hybrid_level": level}
    with torch.cuda.stream(s):
        full = []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)            # light_kd as the benchmark has it: the cue
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
        stream = s.cuda_stream
        plain = lambda p: r.render_volume_device(p, buf.data_ptr(), stream)      # noqa: E731
        over = lambda p: r.render_backdrop_device(p, layer.data_ptr(), far.data_ptr(), buf.data_ptr(), stream)      # noqa: E731

        def pair(twin_key, key):
            out[twin_key + "_ms"], out[twin_key + "_layout"] = time_views(r, plain, full, s.synchronize, 3, a.reps)
            frames = r.backdrop_frames()
            out[key + "_ms"], out[key + "_layout"] = time_views(r, over, full, s.synchronize, 3, a.reps)
            assert r.backdrop_frames() == frames + 8 * (3 + a.reps)
            out[key + "_over_twin_percent"] = [round(100.0 * (b / t - 1.0), 2) for b, t in zip(out[key + "_ms"], out[twin_key + "_ms"])]

        r.set_clip()                                                  # the identity clip: the clipped kernels on the whole segment
        pair("identity_clipped_point", "backdrop")
        r.clear_clip()
        r.set_lighting(*PHONG)
        pair("lit", "backdrop_lit")
        r.set_preintegration()
        pair("slab_lit", "backdrop_slab_lit")
        r.clear_lighting()
        pair("slab", "backdrop_slab")
        r.clear_preintegration()
        # the hybrid against an isosurface frame plus a composite frame of the same view
        iso = lambda p: r.render_iso_device(p, level, 4, buf.data_ptr(), dbuf.data_ptr(), stream)      # noqa: E731
        hybrid = lambda p: r.render_hybrid_device(p, level, 4, buf.data_ptr(), dbuf.data_ptr(), stream)      # noqa: E731
        out["iso_ms"], _ = time_views(r, iso, full, s.synchronize, 3, a.reps)
        out["composite_ms"], out["composite_layout"] = time_views(r, plain, full, s.synchronize, 3, a.reps)
        out["hybrid_ms"], out["hybrid_layout"] = time_views(r, hybrid, full, s.synchronize, 3, a.reps)
        s.synchronize()
        out["hybrid_surface_share"] = round(float((dbuf >= 0).float().mean().item()), 4)
        # the composite pass of the hybrid alone (the hybrid less the isosurface frame) against the backdrop frame that narrows nothing
        out["hybrid_pass_ms"] = [round(h - i, 4) for h, i in zip(out["hybrid_ms"], out["iso_ms"])]
        out["hybrid_pass_against_backdrop_percent"] = [round(100.0 * (hp / b - 1.0), 2) for hp, b in zip(out["hybrid_pass_ms"], out["backdrop_ms"])]
        out["hybrid_against_iso_plus_composite_percent"] = [round(100.0 * (h / (i + c) - 1.0), 2) for h, i, c in zip(out["hybrid_ms"], out["iso_ms"], out["composite_ms"])]
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
