"""Clipped frames against unclipped ones on one GPU, all three projections.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), same build, same process: the full-march
TRILINEAR lit composite, the MIP frame with esl on and the isosurface at level 128 with esl on — each unclipped, clipped by the plane
through the centre that faces the camera (the half of the cube nearer the eye is cut away: n = the view's direction, d = 0) and clipped
by the box [-0.5, 0.5]^3.  The unclipped composite is timed twice: as the product runs it (views 0 / 2 / 3 take the column march) and
under vr_hip_set_brick_plane(9), which declines the column march — what a clipped composite of those views, which reads the quad
bricks, is to be compared with.  Kernel ms per view from vr_hip_timing (hipEvents around the launch).  One JSON object on stdout;
nothing here touches oracle/.

    python scripts/clip_probe.py [--n 1024] [--size 2048] [--reps 5] [--level 128]
"""
import argparse
import importlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_views(r, render, params, clip_of, sync, warm, reps):
    """kernel ms per view; clip_of(p) = keyword arguments of set_clip for that view, or None = no clip"""
    per_view, layouts = [], []
    for p in params:
        clip = clip_of(p)
        if clip is None:
            r.clear_clip()
        else:
            r.set_clip(**clip)
        for _ in range(warm):
            render(p)
        sync()
        r.timing_reset()
        for _ in range(reps):
            render(p)
        sync()
        t = r.timing()
        per_view.append(round(t.kernel_ms_sum / max(1, t.launches), 4))
        layouts.append(r.last_launch()["layout"])
    r.clear_clip()
    return per_view, layouts


def facing_plane(p):
    """the plane through the centre whose kept side is the far half of the cube as seen from the camera"""
    d = [float(x) for x in p.view.direction]
    n = math.sqrt(sum(x * x for x in d))
    return {"plane": (d[0] / n, d[1] / n, d[2] / n, 0.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=float, default=128.0)
    a = ap.parse_args()
    import torch
    vr = importlib.import_module("volume-rendering_amd")
    r = vr.HipRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=r.volume_minmax()[0])
    r.set_transfer_fn(scene.tf, scene.esl)
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    depth = torch.empty((a.size, a.size), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "level": a.level, "library": vr.library_path(), "device": r.device_info()[0]}
    clips = {"unclipped": lambda p: None, "plane": facing_plane, "box": lambda p: {"box_min": (-0.5,) * 3, "box_max": (0.5,) * 3}}
    with torch.cuda.stream(s):
        full, skipping = [], []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)            # lit
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
            q = p.copy()
            q.esl = 1
            skipping.append(q)
        modes = {
            "composite": (lambda p: r.render_volume_device(p, buf.data_ptr(), s.cuda_stream), full),
            "mip_esl1": (lambda p: r.render_mip_device(p, buf.data_ptr(), s.cuda_stream), skipping),
            "iso_esl1": (lambda p: r.render_iso_device(p, a.level, 4, buf.data_ptr(), depth.data_ptr(), s.cuda_stream), skipping),
        }
        for mode, (render, params) in modes.items():
            for name, clip_of in clips.items():
                ms, layouts = time_views(r, render, params, clip_of, s.synchronize, 3, a.reps)
                out[f"{mode}_{name}_ms"], out[f"{mode}_{name}_layout"] = ms, layouts
        r.set_brick_plane(9)                                          # never the column windows
        ms, layouts = time_views(r, modes["composite"][0], full, clips["unclipped"], s.synchronize, 3, a.reps)
        out["composite_unclipped_no_column_ms"], out["composite_unclipped_no_column_layout"] = ms, layouts
        r.set_brick_plane(-1)
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
