"""Depth frames on one GPU: what the alpha-only march costs beside the clipped composite frame it mirrors.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same process, under the
identity clip (the composite then runs raymarch_clipped: the frame a depth frame mirrors, on the copies a depth frame reads):
  * full march (esl = 0, threshold 1.0) and default mode (esl = 1, threshold 0.95): the clipped composite frame, then the depth frame in
    each mode (FIRST at opacity 0.5, PEAK, MEAN) with the alpha buffer and without it (depth alone: a FIRST ray stops at its surface).
    The frames alternate per view, `rounds` times; the spread of a view's ratio over the rounds is the noise floor.
Kernel ms per view from vr_hip_timing (hipEvents around every launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/depth_probe.py [--n 1024] [--size 2048] [--reps 5] [--rounds 2]
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("first", "peak", "mean")


def time_call(r, render, p, sync, warm, reps):
    """mean kernel ms per call of render(p)"""
    for _ in range(warm):
        render(p)
    sync()
    r.timing_reset()
    for _ in range(reps):
        render(p)
    sync()
    return round(r.timing().kernel_ms_sum / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    import torch
    vr = importlib.import_module("volume-rendering_amd")
    r = vr.HipRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=r.volume_minmax()[0])
    r.set_transfer_fn(scene.tf, scene.esl)
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    planes = [torch.empty((a.size, a.size), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "rounds": a.rounds, "device": r.device_info()[0]}
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        r.set_clip()                                                  # the identity clip: raymarch_clipped on the whole segment
        composite = lambda p: r.render_volume_device(p, buf.data_ptr(), stream)      # noqa: E731
        for march in ("full", "default"):
            params = []
            for v in views:
                p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)
                if march == "full":
                    p.esl, p.ray_threshold = 0, 1.0
                params.append(p)
            res = {"composite_clipped_ms": []}
            for mode in MODES:
                res[mode + "_with_alpha_ms"], res[mode + "_depth_alone_ms"] = [], []
            timed = list(res)
            for _ in range(a.rounds):
                row = {k: [] for k in timed}
                for p in params:
                    row["composite_clipped_ms"].append(time_call(r, composite, p, s.synchronize, 2, a.reps))
                    res["composite_layout"] = r.last_launch()["layout"]
                    for mode in MODES:
                        with_alpha = lambda q: r.render_depth_device(q, 0.5, mode, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), stream)      # noqa: E731
                        alone = lambda q: r.render_depth_device(q, 0.5, mode, planes[0].data_ptr(), None, None, stream)      # noqa: E731
                        row[mode + "_with_alpha_ms"].append(time_call(r, with_alpha, p, s.synchronize, 2, a.reps))
                        row[mode + "_depth_alone_ms"].append(time_call(r, alone, p, s.synchronize, 2, a.reps))
                    res["depth_layout"] = r.last_launch()["layout"]
                for k in row:
                    res[k].append(row[k])
            res["over_composite_percent"] = {
                k: [[round(100.0 * (d / c - 1.0), 2) for d, c in zip(dr, cr)] for dr, cr in zip(res[k], res["composite_clipped_ms"])]
                for k in timed if k != "composite_clipped_ms"}
            res["mean_over_views_ms"] = {k: [round(sum(x) / len(x), 4) for x in res[k]] for k in timed}
            out[march] = res
        s.synchronize()
        out["surface_share_of_last_frame"] = round(float((planes[0] >= 0).float().mean().item()), 4)
        out["depth_frames"] = r.depth_frames()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
