"""Fused frames on one GPU: what the second field costs beside the composite and the labelled frames.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same process, under the
identity clip, full march (esl = 0, threshold 1.0) and default mode (esl = 1, threshold 0.95).  B is the volume mirrored along x and z.
  (i)  B silent: the fused frame with weight_b = 0 under A's own leaping bits (its bytes are the composite's: checked) against the clipped
       composite frame and against the labelled frame with all-zero labels and the identity table (the same bytes again) — the second
       gather and the one-sample batch, nothing else;
  (ii) both fields live: B under a hot ramp (16 leading zero entries) with the fused (AND) bits, weights (1, 1), SUM and OVER, unlit and
       lit (vr_hip_set_lighting);
  (iii) the build of B's quad copy: the wall time of the first fused frame (the copy is allocated and built inside it, synchronously) less a
        later one's, beside the kernel time vr_volume_info reports for the same builder on A's quad copy.
The frames alternate per view, `rounds` times; the spread of a view's ratio over the rounds is the noise floor.  Kernel ms per view from
vr_hip_timing (hipEvents around every launch).  A table on stdout, then one JSON object; nothing here touches oracle/.

    python scripts/fused_probe.py [--n 1024] [--size 2048] [--reps 5] [--rounds 2]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHONG = (0.25, 0.65, 0.4, 4)
HOT_ZEROS = 16                                          # more than the 13 of the scene's own function: the background of the shell is transparent in B too


def hot_ramp(zeros=HOT_ZEROS):
    t = np.zeros((128, 4), np.float32)
    for i in range(zeros, 128):
        u = (i - zeros) / float(127 - zeros)
        alpha = 1.0 / 32.0 + 0.5 * u
        t[i] = (min(1.0, 3.0 * u) * alpha, min(1.0, max(0.0, 3.0 * u - 1.0)) * alpha, min(1.0, max(0.0, 3.0 * u - 2.0)) * alpha, alpha)
    return t


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
    fusion = importlib.import_module("volume-rendering_amd.fusion")
    r = fusion.FusedRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    minmax = r.volume_minmax()[0]
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=minmax)
    r.set_transfer_fn(scene.tf, scene.esl)
    out = {"library": os.path.basename(vr.library_path()), "volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "rounds": a.rounds, "device": r.device_info()[0]}
    esl = np.array(scene.esl)
    # B: the volume mirrored along x and z, made on the device; its leaping bits under the hot ramp from the host mirror's builder (the
    # mirror's block extrema are the volume's, mirrored: the shell is symmetric, so the volume's own serve)
    second = torch.from_numpy(r.download_volume()).cuda().flip(0, 2).contiguous()
    hot = hot_ramp()
    scene.set_base_transfer_fn(hot)
    fused_bits = fusion.fused_esl(esl, np.array(scene.esl))
    ones = lambda words: int(sum(bin(int(w)).count("1") for w in words))      # noqa: E731
    out["blocks_marked_empty"] = {"A": ones(esl), "fused": ones(fused_bits)}
    r.set_second_volume(second)
    r.set_labels(torch.zeros((a.n,) * 3, dtype=torch.uint8, device="cuda:0"))
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    other = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    kinds = ("composite_ms", "labelled_ms", "fused_silent_ms", "fused_sum_ms", "fused_over_ms")
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        r.set_clip()                                                  # the identity clip: raymarch_clipped / composite_lit on the whole segment
        composite = lambda p: r.render_volume_device(p, buf.data_ptr(), stream)      # noqa: E731
        labelled = lambda p: r.render_labelled_device(p, other.data_ptr(), stream)   # noqa: E731

        def fused(weight_b, mode):
            return lambda p: r.render_fused_device(p, other.data_ptr(), stream, 1.0, weight_b, mode)
        # (iii) the first fused frame builds B's copy
        p0 = scene.frame_params(views[0], vr.SAMPLE_TRILINEAR)
        r.set_second_transfer_fn(hot, esl)
        composite(p0)
        s.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            fused(0.0, "sum")(p0)
            s.synchronize()
            walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        out["first_fused_frames_wall_ms"] = walls
        out["second_copy_build_ms"] = round(walls[0] - min(walls[1:]), 3)
        out["first_copy_build_ms"] = [round(float(x), 3) for x in r.volume_info().build_ms][:3]      # A's quad copies: the same builder on the same dims
        for shading in ("unlit", "lit"):
            if shading == "lit":
                r.set_lighting(*PHONG)
            else:
                r.clear_lighting()
            for march in ("full", "default"):
                params = []
                for v in views:
                    p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)
                    if march == "full":
                        p.esl, p.ray_threshold = 0, 1.0
                    params.append(p)
                res = {k: [] for k in kinds}
                res["silent_equals_composite"], res["labelled_equals_composite"], res["sum_differs_pixels"] = True, True, []
                for _ in range(a.rounds):
                    row = {k: [] for k in kinds}
                    differs = []
                    for p in params:
                        row["composite_ms"].append(time_call(r, composite, p, s.synchronize, 2, a.reps))
                        row["labelled_ms"].append(time_call(r, labelled, p, s.synchronize, 2, a.reps))
                        res["labelled_equals_composite"] = res["labelled_equals_composite"] and bool(torch.equal(buf, other))
                        r.set_second_transfer_fn(hot, esl)
                        row["fused_silent_ms"].append(time_call(r, fused(0.0, "sum"), p, s.synchronize, 2, a.reps))
                        res["silent_equals_composite"] = res["silent_equals_composite"] and bool(torch.equal(buf, other))
                        r.set_second_transfer_fn(hot, fused_bits)
                        row["fused_sum_ms"].append(time_call(r, fused(1.0, "sum"), p, s.synchronize, 2, a.reps))
                        differs.append(int((buf != other).any(dim=-1).sum().item()))
                        row["fused_over_ms"].append(time_call(r, fused(1.0, "over"), p, s.synchronize, 2, a.reps))
                        res["layout"] = r.last_launch()["layout"]
                    for k in row:
                        res[k].append(row[k])
                    res["sum_differs_pixels"].append(differs)
                res["mean_over_views_ms"] = {k: [round(sum(x) / len(x), 4) for x in res[k]] for k in kinds}
                out[f"{shading}_{march}"] = res
                print(f"{shading}, {march} march: layout {res['layout']}; silent == composite: {res['silent_equals_composite']}; labelled == composite: {res['labelled_equals_composite']}")
                for n in range(a.rounds):
                    print(f"round {n + 1}")
                    print("view  composite   labelled  B silent      %   over labelled %        SUM      %       OVER      %   pixels that differ (SUM)")
                    for v in range(8):
                        c, lab, sil, su, ov = (res[k][n][v] for k in kinds)
                        print(f"{v:4d} {c:10.4f} {lab:10.4f} {sil:10.4f} {100 * (sil / c - 1):+6.1f} {100 * (sil / lab - 1):+17.1f} {su:10.4f} {100 * (su / c - 1):+6.1f} "
                              f"{ov:10.4f} {100 * (ov / c - 1):+6.1f}   {res['sum_differs_pixels'][n][v]}")
                    c, lab, sil, su, ov = (res["mean_over_views_ms"][k][n] for k in kinds)
                    print(f"mean {c:10.4f} {lab:10.4f} {sil:10.4f} {100 * (sil / c - 1):+6.1f} {100 * (sil / lab - 1):+17.1f} {su:10.4f} {100 * (su / c - 1):+6.1f} "
                          f"{ov:10.4f} {100 * (ov / c - 1):+6.1f}")
                print(flush=True)
        s.synchronize()
        out["fused_frames"] = r.fused_frames()
    print(f"first three fused frames of the context, wall ms: {out['first_fused_frames_wall_ms']}: B's quad copy is allocated and built inside the first — "
          f"{out['second_copy_build_ms']} ms more than a later one; kernel ms of the same builder on A's quad copies (vr_volume_info build_ms, planes xy / xz / yz): {out['first_copy_build_ms']}")
    print(f"blocks marked empty: A's bits {out['blocks_marked_empty']['A']}, the fused bits {out['blocks_marked_empty']['fused']}")
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
