"""Labelled composite frames on one GPU: what the label gather and the table entry cost beside the clipped composite frame.

C4 (shell 1024^3, 1 byte per voxel, 2048 x 2048, the reference's eight benchmark views), TRILINEAR, same build, same process, under the
identity clip (the composite then runs raymarch_clipped: the frame a labelled frame is defined by, which this feature leaves byte-identical):
  * full march (esl = 0, threshold 1.0) and default mode (esl = 1, threshold 0.95): the clipped composite frame, then the labelled frame
    with an all-identity table (its bytes are the composite's: checked) and with the structured table (identity, hidden, mix 1, a
    fractional mix, a fractional opacity over slanted stripes and a ball).  The frames alternate per view, `rounds` times; the spread of a
    view's ratio over the rounds is the noise floor.
The form of the label fetch is the build's: the product fetches the label of the samples that survive both transparency shortcuts (a
dependent load); `scripts/build_variant.sh label_early -DVR_LABEL_EARLY` issues it with the batch for every sample — run this script once
per library (VR_HIP_LIB=build_variants/libvr_hip_label_early.so for the second).
Kernel ms per view from vr_hip_timing (hipEvents around every launch).  One JSON object on stdout; nothing here touches oracle/.

    python scripts/label_probe.py [--n 1024] [--size 2048] [--reps 5] [--rounds 2]
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# entry i of the structured table: identity, hidden, mix 1, a fractional mix, a fractional opacity with a mix
STRUCTURED = ((0.0, 0.0, 0.0, 0.0, 1.0), (0.25, 0.5, 0.75, 0.5, 0.0), (0.9, 0.2, 0.1, 1.0, 1.0), (0.1, 0.8, 0.3, 0.5, 1.0), (0.2, 0.4, 1.0, 0.25, 0.5))


def structured_labels(torch, n):
    """(n, n, n) uint8 on the device: slanted stripes five voxels thick along (3, 2, 1) carrying 0..3, a ball of radius n / 3 carrying 4"""
    lab = torch.empty((n, n, n), dtype=torch.uint8, device="cuda:0")
    x = torch.arange(n, dtype=torch.int32, device="cuda:0")[None, :]
    y = torch.arange(n, dtype=torch.int32, device="cuda:0")[:, None]
    c, r2 = (n - 1) / 2.0, (n / 3.0) ** 2
    d2 = (x.float() - c) ** 2 + (y.float() - c) ** 2
    for z in range(n):
        plane = (((3 * x + 2 * y + z) // 5) % 4).to(torch.uint8)
        plane[d2 + (z - c) ** 2 <= r2] = 4
        lab[z] = plane
    return lab


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
    labels = structured_labels(torch, a.n)
    torch.cuda.synchronize()
    r.set_labels(labels)
    del labels
    views = [vr.benchmark_view(a.size, a.size, i) for i in range(8)]
    buf = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    other = torch.empty((a.size, a.size, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    out = {"library": os.path.basename(vr.library_path()), "volume": [a.n] * 3, "viewport": [a.size, a.size], "reps": a.reps, "rounds": a.rounds, "device": r.device_info()[0]}
    kinds = ("composite_clipped_ms", "labelled_identity_ms", "labelled_structured_ms")
    with torch.cuda.stream(s):
        stream = s.cuda_stream
        r.set_clip()                                                  # the identity clip: raymarch_clipped on the whole segment
        composite = lambda p: r.render_volume_device(p, buf.data_ptr(), stream)      # noqa: E731
        labelled = lambda p: r.render_labelled_device(p, other.data_ptr(), stream)   # noqa: E731
        for march in ("full", "default"):
            params = []
            for v in views:
                p = scene.frame_params(v, vr.SAMPLE_TRILINEAR)
                if march == "full":
                    p.esl, p.ray_threshold = 0, 1.0
                params.append(p)
            res = {k: [] for k in kinds}
            res["identity_equals_composite"], res["structured_differs_pixels"] = True, []
            for _ in range(a.rounds):
                row = {k: [] for k in kinds}
                differs = []
                for p in params:
                    row["composite_clipped_ms"].append(time_call(r, composite, p, s.synchronize, 2, a.reps))
                    res["composite_layout"] = r.last_launch()["layout"]
                    r.set_label_table(None)
                    row["labelled_identity_ms"].append(time_call(r, labelled, p, s.synchronize, 2, a.reps))
                    res["identity_equals_composite"] = res["identity_equals_composite"] and bool(torch.equal(buf, other))
                    r.set_label_table(STRUCTURED)
                    row["labelled_structured_ms"].append(time_call(r, labelled, p, s.synchronize, 2, a.reps))
                    differs.append(int((buf != other).any(dim=-1).sum().item()))
                    res["labelled_layout"] = r.last_launch()["layout"]
                for k in row:
                    res[k].append(row[k])
                res["structured_differs_pixels"].append(differs)
            res["over_composite_percent"] = {
                k: [[round(100.0 * (d / c - 1.0), 2) for d, c in zip(dr, cr)] for dr, cr in zip(res[k], res["composite_clipped_ms"])]
                for k in kinds if k != "composite_clipped_ms"}
            res["mean_over_views_ms"] = {k: [round(sum(x) / len(x), 4) for x in res[k]] for k in kinds}
            out[march] = res
        s.synchronize()
        out["labelled_frames"] = r.labelled_frames()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
