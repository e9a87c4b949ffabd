"""Shaded isosurface frames against the MIP frame and the default-mode composite on one GPU.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same view: the
isosurface frame with esl off (every march sample fetched) and esl on (fetches skipped by the one-bit block table) at levels inside the
shell's range and at one above the volume's maximum (esl on: every fetch skipped, the frame is the pure cost of marching k), lit and
with depth; beside it the MIP frame with esl on and the composite in the default mode (ESL + ERT, lit).  Kernel ms per view from
vr_hip_timing (hipEvents around the launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/iso_probe.py [--n 1024] [--size 2048] [--reps 5] [--refine 4] [--levels 128 220 300] [--light-kd <kd>]

--refine 0 --light-kd 0 leaves the march and the two stores: the difference to the default run is what bisection and gradient cost."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_frames(r, render, params, sync, warm, reps):
    per_view = []
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
    return per_view


def with_esl(params, esl, light_kd=None):
    out = []
    for p in params:
        q = p.copy()
        q.esl = esl
        if light_kd is not None:
            q.light_kd = light_kd
        out.append(q)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--levels", type=float, nargs="+", default=[128.0, 220.0, 300.0])
    ap.add_argument("--light-kd", type=float, default=None, help="light_kd of the isosurface frames (default: the scene's)")
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
    out = {"volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "refine": a.refine, "library": vr.library_path(), "device": r.device_info()[0]}
    with torch.cuda.stream(s):
        ps = [scene.frame_params(v, vr.SAMPLE_TRILINEAR) for v in views]         # the default mode: ESL + ERT, lit
        out["light_kd"] = round(float(ps[0].light_kd), 4)
        out["iso_light_kd"] = out["light_kd"] if a.light_kd is None else a.light_kd
        out["dvr_default_ms"] = time_frames(r, lambda p: r.render_volume_device(p, buf.data_ptr(), s.cuda_stream), ps, s.synchronize, 4, a.reps)
        out["mip_esl1_ms"] = time_frames(r, lambda p: r.render_mip_device(p, buf.data_ptr(), s.cuda_stream), with_esl(ps, 1), s.synchronize, 2, a.reps)
        for level in a.levels:
            e = {}
            for esl in (0, 1):
                e[f"iso_esl{esl}_ms"] = time_frames(r, lambda p: r.render_iso_device(p, level, a.refine, buf.data_ptr(), depth.data_ptr(), s.cuda_stream),
                                                    with_esl(ps, esl, a.light_kd), s.synchronize, 2, a.reps)
            e["surface_pixels"] = []
            for p in with_esl(ps, 1):
                r.render_iso_device(p, level, a.refine, buf.data_ptr(), depth.data_ptr(), s.cuda_stream)
                s.synchronize()
                e["surface_pixels"].append(int((depth >= 0).sum().item()))
            e["layout"] = r.last_launch()["layout"]
            out[f"level_{level:g}"] = e
        for k in [k for k in out if k.endswith("_ms")]:
            out[k.replace("_ms", "_mean_ms")] = round(sum(out[k]) / len(out[k]), 4)
        for level in a.levels:
            e = out[f"level_{level:g}"]
            for esl in (0, 1):
                e[f"iso_esl{esl}_mean_ms"] = round(sum(e[f"iso_esl{esl}_ms"]) / 8, 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
