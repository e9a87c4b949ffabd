"""Light-source shadows on one GPU: what the light grid costs to build and what the factor fetch costs per frame.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), full-march TRILINEAR lit composite, same build,
same process:
  * build time of the light grid at S = 64 / 128 / 256 with step = ray_step (vr_hip_shadow_builds: hipEvents around the builder);
  * the shadowed frame against the same frame with the shadow cleared, which then runs the unshadowed kernels (views 0 / 2 / 3: the column
    march);
  * the shadowed frame against the identity-clipped frame, its nearest twin — the same copies, the same march, clip_segment included: that
    difference is the price of the factor fetch (and of the one sample less of prefetch) alone.
The light of the grid is the views' own light.  Kernel ms per view from vr_hip_timing (hipEvents around the launch).  One JSON object on
stdout; nothing here touches oracle/.

    python scripts/shadow_probe.py [--n 1024] [--size 2048] [--reps 5] [--dims 128]
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_views(r, render, params, sync, warm, reps):
    per_view, layouts = [], []
    for p in params:
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
    return per_view, layouts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, default=128, help="S of the grid the frames are timed with")
    a = ap.parse_args()
    import torch
    vr = importlib.import_module("volume-rendering_amd")
    r = vr.HipRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=r.volume_minmax()[0])
    r.set_transfer_fn(scene.tf, scene.esl)
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "library": vr.library_path(), "device": r.device_info()[0]}
    with torch.cuda.stream(s):
        full = []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)            # lit
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
        light, step = tuple(full[0].view.light_pos), float(full[0].ray_step)
        out["light"], out["step"] = list(light), step
        r.prepare(vr.COPY_QUAD_XY)                                    # the builder's copy: not part of the build time below
        build = {}
        for dims in (64, 128, 256):
            ms = []
            for rep in range(3):
                r.clear_shadow()
                r.set_shadow(light, dims, step)
                q = r.download_shadow()
                ms.append(round(r.shadow_builds()[1], 4))
            build[str(dims)] = {"build_ms": ms, "black_percent": round(100.0 * float((q == 0).mean()), 1), "lit_percent": round(100.0 * float((q == 255).mean()), 1)}
        out["grid"] = build
        render = lambda p: r.render_volume_device(p, buf.data_ptr(), s.cuda_stream)      # noqa: E731
        r.clear_shadow()
        out["unshadowed_ms"], out["unshadowed_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.set_clip()                                                  # the identity clip: the clipped kernels on the whole segment
        out["identity_clipped_ms"], out["identity_clipped_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.clear_clip()
        r.set_shadow(light, a.dims, step)
        out["shadowed_ms"], out["shadowed_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        out["shadowed_dims"] = a.dims
        r.clear_shadow()
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
