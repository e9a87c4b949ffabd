"""2D transfer-function frames on one GPU: what the second classification axis costs beside the composite frames it is defined by, and the
gradient histogram beside the 1-D one.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same process, under the
identity clip, full march (esl = 0, threshold 1.0) and default mode (esl = 1, threshold 0.95):
  (i)  unlit: the clipped composite frame against the tf2d frame whose rows all equal the transfer function (its bytes are the
       composite's: checked) — the price of the family's shape with the second dimension unused — and against the structured table;
  (ii) lit (vr_hip_set_lighting): composite_lit against the tf2d frame with the equal rows and with the structured table — the price of
       the gradient for samples that are not dense.
The structured table: five rows over the scene's function in bands of 16 entries — every row the function in the even bands; the function,
half of it, zero and a two-row colour ramp in the odd ones —, g_scale = 4 / G, G the gradient magnitude a tenth of the moving voxels exceed
(from the device's own histogram).  The frames alternate per view, `rounds` times; the spread of a view's ratio over the rounds is the
noise floor.  Then vr_hip_gradient_histogram (5 and 32 rows) and vr_hip_volume_histogram on the same volume, in GB/s of the linear array.
Kernel ms per view from vr_hip_timing (hipEvents around every launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/tf2d_probe.py [--n 1024] [--size 2048] [--reps 5] [--rounds 2]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHONG = (0.25, 0.65, 0.4, 4)


def structured_table(tf):
    tf = np.ascontiguousarray(tf, np.float32).reshape(128, 4)
    t = np.repeat(tf[None], 5, axis=0).copy()
    for i in range(128):
        if (i // 16) % 2 == 0:
            continue
        r = ((5 * i + 3) % 64) / 64.0
        t[1, i] = tf[i] * np.float32(0.5)
        t[2, i] = 0.0
        t[3, i] = (0.25 * r, 0.25 * 0.5, 0.25 * (1.0 - r), 0.25)
        t[4, i] = (0.5 * (1.0 - r), 0.5 * r, 0.5 * 0.75, 0.5)
    return t


def choose_g_scale(r, n):
    bound = 255.0 * 0.5 * n * 3.0 ** 0.5
    first = r.gradient_histogram(32, 31.0 / bound).sum(axis=1)
    top = (int(np.nonzero(first)[0].max()) + 0.5) * bound / 31.0
    moving = r.gradient_histogram(32, 31.0 / top).sum(axis=1).astype(np.int64)
    moving[0] = 0
    tail = np.cumsum(moving[::-1])[::-1]
    row = int(np.nonzero(tail * 10 >= moving.sum())[0].max())
    return float(2.0 ** round(np.log2(4.0 / (max(row, 1) * top / 31.0))))


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
    tf2d = importlib.import_module("volume-rendering_amd.tf2d")
    r = tf2d.Tf2dRenderer(0)
    r.generate_volume("shell", a.n, seed=1, bytes_per_voxel=1)
    minmax = r.volume_minmax()[0]
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=minmax)
    r.set_transfer_fn(scene.tf, scene.esl)
    out = {"library": os.path.basename(vr.library_path()), "volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "rounds": a.rounds, "device": r.device_info()[0]}

    # the histograms first: the gradient histogram also places the rows
    gigabytes = a.n ** 3 / 1e9
    g_scale = choose_g_scale(r, a.n)
    hist = {"g_scale": g_scale}
    for bins in (5, 32):
        ms = []
        for _ in range(1 + a.reps):
            h = r.gradient_histogram(bins, g_scale * bins / 5.0)
            ms.append(r.last_gradient_histogram_ms)
        hist[f"gradient_{bins}_rows_ms"] = [round(m, 4) for m in ms[1:]]
        hist[f"gradient_{bins}_rows_gb_s"] = round(gigabytes / (min(ms[1:]) * 1e-3), 1)
        hist[f"gradient_{bins}_rows_share"] = [round(float(x) / a.n ** 3, 4) for x in h.sum(axis=1)]
    plain = [r.volume_histogram() for _ in range(1 + a.reps)][1:]
    hist["volume_histogram_ms"] = [round(ms, 4) for _, ms in plain]
    hist["volume_histogram_gb_s"] = round(gigabytes / (min(ms for _, ms in plain) * 1e-3), 1)
    hist["row_sum_equals_volume_histogram"] = bool(np.array_equal(h.sum(axis=0), plain[0][0]))
    out["histogram"] = hist

    equal = np.repeat(np.asarray(scene.tf, np.float32).reshape(1, 128, 4), 5, axis=0)
    structured = structured_table(scene.tf)
    # the leaping bits of the structured table: the host mirror's builder on the envelope (it reads the alpha channel alone)
    esl = np.array(scene.esl)
    scene.set_base_transfer_fn(tf2d.envelope(structured))
    structured_esl = np.array(scene.esl)
    out["blocks_marked_empty"] = {"function": int(sum(bin(int(w)).count("1") for w in esl)), "structured_envelope": int(sum(bin(int(w)).count("1") for w in structured_esl))}
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    other = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    kinds = ("composite_ms", "tf2d_equal_rows_ms", "tf2d_structured_ms")
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        r.set_clip()                                                  # the identity clip: raymarch_clipped / composite_lit on the whole segment
        composite = lambda p: r.render_volume_device(p, buf.data_ptr(), stream)      # noqa: E731
        frame = lambda p: r.render_tf2d_device(p, other.data_ptr(), stream)          # noqa: E731
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
                res["equal_rows_equal_composite"], res["structured_differs_pixels"] = True, []
                for _ in range(a.rounds):
                    row = {k: [] for k in kinds}
                    differs = []
                    for p in params:
                        row["composite_ms"].append(time_call(r, composite, p, s.synchronize, 2, a.reps))
                        r.set_tf2d(equal, g_scale, esl)
                        row["tf2d_equal_rows_ms"].append(time_call(r, frame, p, s.synchronize, 2, a.reps))
                        res["equal_rows_equal_composite"] = res["equal_rows_equal_composite"] and bool(torch.equal(buf, other))
                        r.set_tf2d(structured, g_scale, structured_esl)
                        row["tf2d_structured_ms"].append(time_call(r, frame, p, s.synchronize, 2, a.reps))
                        differs.append(int((buf != other).any(dim=-1).sum().item()))
                        res["tf2d_layout"] = r.last_launch()["layout"]
                    for k in row:
                        res[k].append(row[k])
                    res["structured_differs_pixels"].append(differs)
                res["over_composite_percent"] = {
                    k: [[round(100.0 * (d / c - 1.0), 2) for d, c in zip(dr, cr)] for dr, cr in zip(res[k], res["composite_ms"])]
                    for k in kinds if k != "composite_ms"}
                res["mean_over_views_ms"] = {k: [round(sum(x) / len(x), 4) for x in res[k]] for k in kinds}
                out[f"{shading}_{march}"] = res
        s.synchronize()
        out["tf2d_frames"] = r.tf2d_frames()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
