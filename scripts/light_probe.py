"""Gradient lighting on one GPU: what Blinn-Phong from the field's gradient costs per frame.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), full-march TRILINEAR composite, same build, same
process:
  * the gradient-lit frame against the identity-clipped cue-lit frame, its nearest twin — the same copies, the same march, clip_segment
    included: that difference is the price of the six gradient fetches of a dense sample (and of the one sample less of prefetch) alone;
  * the same two with a shadow at S = 128 (the twin is then the shadowed cue-lit frame);
  * beside them the cue-lit frame with neither clip nor lighting, which runs the run-brick and column marches.
The dense-sample share is taken from the volume's histogram: the share of voxels whose value the transfer function gives an alpha above
0.05 — what a full march, which samples the cube evenly, lights.  Kernel ms per view from vr_hip_timing (hipEvents around the launch).
One JSON object on stdout; nothing here touches oracle/.

    python scripts/light_probe.py [--n 1024] [--size 2048] [--reps 5] [--dims 128]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHONG = (0.25, 0.65, 0.4, 4)


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
    ap.add_argument("--dims", type=int, default=128, help="S of the light grid of the shadowed pair")
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
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "device": r.device_info()[0], "lighting": list(PHONG)}
    # alpha of the filtered lookup at every voxel value 0..255 (the arithmetic of a composited sample's lookup, in double)
    tf = np.asarray(scene.tf, np.float64).reshape(128, 4)
    tb = np.clip(np.arange(256) * (128.0 / 255.0) - 0.5, 0.0, 127.0)
    i0 = np.minimum(tb.astype(int), 127)
    i1 = np.minimum(i0 + 1, 127)
    alpha = tf[i0, 3] + (tb - i0) * (tf[i1, 3] - tf[i0, 3])
    hist = np.asarray(r.volume_histogram()[0], np.float64)
    out["dense_voxel_percent"] = round(100.0 * float(hist[alpha > 0.05].sum() / hist.sum()), 2)
    with torch.cuda.stream(s):
        full = []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)            # light_kd as the benchmark has it: the cue
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
        light, step = tuple(full[0].view.light_pos), float(full[0].ray_step)
        render = lambda p: r.render_volume_device(p, buf.data_ptr(), s.cuda_stream)      # noqa: E731
        out["cue_ms"], out["cue_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.set_clip()                                                  # the identity clip: the clipped kernels on the whole segment
        out["identity_clipped_cue_ms"], out["identity_clipped_cue_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.clear_clip()
        r.set_lighting(*PHONG)
        frames = r.lighting_frames()
        out["lit_ms"], out["lit_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        assert r.lighting_frames() == frames + 8 * (3 + a.reps)
        r.clear_lighting()
        r.set_shadow(light, a.dims, step)
        out["shadowed_cue_ms"], out["shadowed_cue_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.set_lighting(*PHONG)
        out["shadowed_lit_ms"], out["shadowed_lit_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        out["shadow_dims"] = a.dims
        r.clear_lighting()
        r.clear_shadow()
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
