"""Section frames on one GPU: what the section march costs beside the MIP march, a POINT frame, and the in-volume call.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same process:
  * a MAX section facing the view whose slab contains the whole cube (h = 4: nothing is narrowed, every ray marches its whole segment and
    carries maximum, minimum, sum and count) against the MIP frame under the identity clip with esl = 0 — the same copies, the same
    march, clip_segment included.  The two alternate per view, `rounds` times; the ratio is reported per view and round, and the spread
    of a view's ratio over the rounds is the noise floor the ratios are read against;
  * a POINT frame of the face-on plane through the centre, with and without a depth buffer;
  * the in-volume call (one vr_hip_render_section_in_volume_device: the section frame, then the backdrop frame in place) against the
    section frame and a plain backdrop frame issued separately, for that POINT section and the full-march composite.
Kernel ms per view from vr_hip_timing (hipEvents around every launch; an in-volume call is two launches).  One JSON object on stdout;
nothing here touches oracle/.

    python scripts/section_probe.py [--n 1024] [--size 2048] [--reps 5] [--rounds 2]
"""
import argparse
import importlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_call(r, render, p, sync, warm, reps):
    """mean kernel ms per call of render(p) (a call may be several launches)"""
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
    dbuf = torch.empty((a.size, a.size), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "rounds": a.rounds, "device": r.device_info()[0]}
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        full, facing = [], []
        for v in views:
            p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)
            p.esl, p.ray_threshold = 0, 1.0                           # the full march
            full.append(p)
            d = [float(c) for c in v.direction]
            norm = math.sqrt(sum(c * c for c in d))
            facing.append((d[0] / norm, d[1] / norm, d[2] / norm, 0.0))
        r.set_clip()                                                  # the identity clip: mip_clipped on the whole segment
        mip = lambda p: r.render_mip_device(p, buf.data_ptr(), stream)      # noqa: E731
        out["mip_ms"], out["section_max_ms"], out["section_over_mip_percent"] = [], [], []
        for _ in range(a.rounds):
            mip_ms, sec_ms = [], []
            for p, plane in zip(full, facing):
                whole = lambda q: r.render_section_device(q, plane, 4.0, "max", None, buf.data_ptr(), None, stream)      # noqa: E731
                mip_ms.append(time_call(r, mip, p, s.synchronize, 2, a.reps))
                sec_ms.append(time_call(r, whole, p, s.synchronize, 2, a.reps))
            out["mip_layout"] = r.last_launch()["layout"]
            out["mip_ms"].append(mip_ms)
            out["section_max_ms"].append(sec_ms)
            out["section_over_mip_percent"].append([round(100.0 * (b / t - 1.0), 2) for b, t in zip(sec_ms, mip_ms)])
        ratios = out["section_over_mip_percent"]
        out["ratio_spread_between_rounds_percent"] = [round(max(x[v] for x in ratios) - min(x[v] for x in ratios), 2) for v in range(8)]
        r.clear_clip()
        point_ms, point_depth_ms, separate_ms, in_volume_ms, backdrop_ms = [], [], [], [], []
        for p, plane in zip(full, facing):
            point = lambda q: r.render_section_device(q, plane, 0.0, "point", None, buf.data_ptr(), None, stream)      # noqa: E731
            with_depth = lambda q: r.render_section_device(q, plane, 0.0, "point", None, buf.data_ptr(), dbuf.data_ptr(), stream)      # noqa: E731
            inside = lambda q: r.render_section_in_volume_device(q, plane, 0.0, "point", None, buf.data_ptr(), dbuf.data_ptr(), stream)      # noqa: E731

            def separate(q):
                r.render_section_device(q, plane, 0.0, "point", None, buf.data_ptr(), dbuf.data_ptr(), stream)
                r.render_backdrop_device(q, buf.data_ptr(), dbuf.data_ptr(), buf.data_ptr(), stream)
            point_ms.append(time_call(r, point, p, s.synchronize, 2, a.reps))
            point_depth_ms.append(time_call(r, with_depth, p, s.synchronize, 2, a.reps))
            separate_ms.append(time_call(r, separate, p, s.synchronize, 2, a.reps))
            in_volume_ms.append(time_call(r, inside, p, s.synchronize, 2, a.reps))
            backdrop_ms.append(round(in_volume_ms[-1] - point_depth_ms[-1], 4))
        out.update(point_ms=point_ms, point_with_depth_ms=point_depth_ms, section_then_backdrop_ms=separate_ms, in_volume_ms=in_volume_ms,
                   in_volume_composite_pass_ms=backdrop_ms,
                   in_volume_against_separate_percent=[round(100.0 * (i / t - 1.0), 2) for i, t in zip(in_volume_ms, separate_ms)])
        s.synchronize()
        out["section_share_of_last_view"] = round(float((dbuf >= 0).float().mean().item()), 4)
        out["section_frames"] = r.section_frames()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
