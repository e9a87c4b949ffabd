"""Maximum-intensity projection against the full-march composite on one GPU.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), NEAREST and TRILINEAR, same build, same
view, same sampling: the full-march DVR frame (esl off, threshold 1, lit) that scripts/bench_extras.py times, the MIP frame with
esl off (every sample fetched) and with esl on (fetches skipped by block maxima, rays stopped at the volume's maximum).  Kernel
ms per view from vr_hip_timing (hipEvents around the launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/mip_probe.py [--n 1024] [--size 2048] [--reps 5] [--bytes 1]

With a library built with `make EXTRA=-DVR_MIP_STATS` (scripts/build_variant.sh mipstats -DVR_MIP_STATS, then VR_HIP_LIB=...) the
esl-on frames also report the fraction of fetches they skipped; that build's times are not the product's."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_frames(r, render, params, buf, stream, sync, warm, reps):
    per_view = []
    for p in params:
        for _ in range(warm):
            render(p, buf.data_ptr(), stream)
        sync()
        r.timing_reset()
        for _ in range(reps):
            render(p, buf.data_ptr(), stream)
        sync()
        t = r.timing()
        per_view.append(round(t.kernel_ms_sum / max(1, t.launches), 4))
    return per_view


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1)
    a = ap.parse_args()
    import torch
    vr = importlib.import_module("volume-rendering_amd")
    L = vr.lib()
    stats_fn = getattr(L, "vr_hip_debug_mip_stats", None)      # only in the -DVR_MIP_STATS build
    if stats_fn is not None:
        stats_fn.restype, stats_fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    r = vr.HipRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=a.bytes)
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=r.volume_minmax()[0])
    r.set_transfer_fn(scene.tf, scene.esl)
    scene.set_modes(esl=False, ray_threshold=1.0)
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"volume": [a.n] * 3, "bytes_per_voxel": a.bytes, "viewport": [a.size, a.size], "reps": a.reps, "library": vr.library_path(),
           "stats_build": stats_fn is not None, "device": r.device_info()[0]}
    with torch.cuda.stream(s):
        for name, code in (("nearest", vr.SAMPLE_NEAREST), ("trilinear", vr.SAMPLE_TRILINEAR)):
            ps = [scene.frame_params(v, code) for v in views]
            ps_on = []
            for p in ps:
                q = p.copy()
                q.esl = 1
                ps_on.append(q)
            e = {"dvr_full_march_ms": time_frames(r, r.render_volume_device, ps, buf, s.cuda_stream, s.synchronize, 4, a.reps)}
            e["dvr_layouts"] = []
            for p in ps:
                r.render_volume_device(p, buf.data_ptr(), s.cuda_stream)
                e["dvr_layouts"].append(r.last_launch()["layout"])
            e["mip_esl0_ms"] = time_frames(r, r.render_mip_device, ps, buf, s.cuda_stream, s.synchronize, 2, a.reps)
            e["mip_esl1_ms"] = time_frames(r, r.render_mip_device, ps_on, buf, s.cuda_stream, s.synchronize, 2, a.reps)
            e["mip_layouts"] = []
            for p in ps:
                r.render_mip_device(p, buf.data_ptr(), s.cuda_stream)
                e["mip_layouts"].append(r.last_launch()["layout"])
            s.synchronize()
            if stats_fn is not None:
                two = (C.c_uint64 * 2)()
                stats_fn(r._ctx, two)                      # reset
                e["fetches_skipped_fraction"] = []
                for q in ps_on:
                    r.render_mip_device(q, buf.data_ptr(), s.cuda_stream)
                    s.synchronize()
                    stats_fn(r._ctx, two)
                    e["fetches_skipped_fraction"].append(round(1.0 - two[1] / max(1, two[0]), 4))
            for k in ("dvr_full_march_ms", "mip_esl0_ms", "mip_esl1_ms"):
                e[k.replace("_ms", "_mean_ms")] = round(sum(e[k]) / len(e[k]), 4)
            out[name] = e
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
