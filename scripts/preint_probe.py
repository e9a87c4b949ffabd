"""Pre-integrated classification on one GPU: what the slab lookup costs per frame.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), full-march TRILINEAR composite, same build, same
process:
  * the slab frame against the identity-clipped point-classified frame, its nearest twin — the same copies, the same march, clip_segment
    included: that difference is the price of the previous coordinate (shortcut variant (a): a copy of the previous slot and its lazy
    resolution; variant (b), -DVR_SLAB_LAZY=0: every sample resolved), of the integral lookups of the wide slabs and of the one sample
    less of prefetch;
  * the same under the lighting { 0.25, 0.65, 0.4, 4 } against the gradient-lit frame;
  * beside them the point-classified frame with no state set, which runs the run-brick and column marches.
Kernel ms per view from vr_hip_timing (hipEvents around the launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/preint_probe.py [--n 1024] [--size 2048] [--reps 5] [--variant a]
"""
import argparse
import importlib
import json
import os
import sys

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
    ap.add_argument("--variant", default="a", help="label of the shortcut variant the library was built with: a (the default build) or b (-DVR_SLAB_LAZY=0)")
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
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "device": r.device_info()[0], "lighting": list(PHONG),
           "shortcut_variant": a.variant}
    with torch.cuda.stream(s):
        full = []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)            # light_kd as the benchmark has it: the cue
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
        render = lambda p: r.render_volume_device(p, buf.data_ptr(), s.cuda_stream)      # noqa: E731
        out["point_ms"], out["point_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.set_clip()                                                  # the identity clip: the clipped kernels on the whole segment
        out["identity_clipped_point_ms"], out["identity_clipped_point_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.clear_clip()
        r.set_preintegration()
        frames = r.preint_frames()
        out["slab_ms"], out["slab_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        assert r.preint_frames() == frames + 8 * (3 + a.reps)
        r.set_lighting(*PHONG)
        out["slab_lit_ms"], out["slab_lit_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.clear_preintegration()
        out["lit_ms"], out["lit_layout"] = time_views(r, render, full, s.synchronize, 3, a.reps)
        r.clear_lighting()
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
