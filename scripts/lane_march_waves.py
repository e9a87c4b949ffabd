#!/usr/bin/env python3
"""Which waves of a column frame march per lane?  CPU only.

col_wave_eligibility (csrc/vr_kernels.hip) sends a wave to the per-lane march when its live lanes do not share kx bit for bit.  This
replays pixel_ray and intersect (csrc/vr_march.h) for every pixel of a view in numpy float32 — the same operations in the same order, one
rounding each: the library is built with -ffp-contract=off — and lists the 8x8-pixel waves whose live lanes carry more than one kx.  The
view comes from the host library (vr_host_benchmark_view_index / vr_host_benchmark_view), as for a frame that is rendered.

    python scripts/lane_march_waves.py --viewport 2048 --views 0,2,3
    python scripts/lane_march_waves.py --viewport 64 --pose 180,90,0

Orthogonal views, whole frames (one band), the default ray step guard left out (ky + step > ky holds for every segment of the cube).
--phase px,py shifts the tiles as the kernels' tile phase does (the wave at (wx, wy) starts at pixel (8 wx - px, 8 wy - py))."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F = np.float32


def pixel_segments(view):
    """(kx, ky, alive) of every pixel of an orthogonal view, [row, column]: pixel_ray<ORTHOGONAL> and intersect, operation by operation."""
    w, h = int(view.width), int(view.height)
    fx = (np.arange(w, dtype=np.int64) - w // 2).astype(F)[None, :]
    fy = (np.arange(h, dtype=np.int64) - h // 2).astype(F)[:, None]
    vo, vd, vr_, vu = ([F(x[i]) for i in range(3)] for x in (view.origin, view.direction, view.right_plane, view.up_plane))
    lo, hi = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(3):
            origin = (vo[c] + vr_[c] * fx) + vu[c] * fy                      # two roundings per product-sum: no fused multiply-add
            d = vd[c] if vd[c] != 0 else F(0.00001)
            k1, k2 = (F(-1.0) - origin) / d, (F(1.0) - origin) / d
            lo.append(np.where(k1 < k2, k1, k2))                             # flmin / flmax: a < b ? a : b, a > b ? a : b
            hi.append(np.where(k1 > k2, k1, k2))
    fmax = lambda a, b: np.where(a > b, a, b)
    fmin = lambda a, b: np.where(a < b, a, b)
    kx = fmax(fmax(lo[0], lo[1]), lo[2])
    ky = fmin(fmin(hi[0], hi[1]), hi[2])
    kx = fmax(kx, F(0))
    kx, ky = np.broadcast_to(kx, (h, w)).astype(F), np.broadcast_to(ky, (h, w)).astype(F)
    return kx, ky, (kx < ky) & (ky > 0)


def mixed_entry_waves(view, phase=(0, 0)):
    """[(wave column, wave row, distinct kx among the live lanes)] of the waves whose live lanes do not share kx bit for bit."""
    kx, _, alive = pixel_segments(view)
    h, w = kx.shape
    bits = kx.view(np.uint32)
    px, py = phase
    found = []
    for wy in range((h + py + 7) // 8):
        y0, y1 = max(0, 8 * wy - py), min(h, 8 * wy - py + 8)
        if y0 >= y1:
            continue
        for wx in range((w + px + 7) // 8):
            x0, x1 = max(0, 8 * wx - px), min(w, 8 * wx - px + 8)
            if x0 >= x1:
                continue
            live = bits[y0:y1, x0:x1][alive[y0:y1, x0:x1]]
            if live.size and (live != live.flat[0]).any():
                found.append((wx, wy, int(np.unique(live).size)))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--viewport", type=int, default=2048)
    ap.add_argument("--views", default="0,2,3", help="benchmark views (0-3 are orthogonal)")
    ap.add_argument("--pose", default="", help="instead of --views: 'ax,ay,az' camera angles in degrees at distance 2; several separated by ';'")
    ap.add_argument("--phase", default="0,0", help="tile phase px,py")
    a = ap.parse_args()
    vr = importlib.import_module("volume-rendering_amd")
    phase = tuple(int(x) for x in a.phase.split(","))
    W = a.viewport
    poses = [tuple(float(x) for x in q.split(",")) for q in a.pose.split(";") if q]
    views = [(f"pose {p}", vr.custom_view(W, W, False, p, 2.0)) for p in poses] if poses else [(f"view {int(v)}", vr.benchmark_view(W, W, int(v))) for v in a.views.split(",")]
    for name, view in views:
        if view.perspective:
            print(json.dumps({"view": name, "skipped": "perspective"}))
            continue
        waves = mixed_entry_waves(view, phase)
        rows = sorted({wy for _, wy, _ in waves})
        print(json.dumps({"view": name, "viewport": W, "phase": phase, "waves": ((W + 7) // 8) ** 2, "mixed_entry_waves": len(waves), "wave_rows": rows,
                          "pixel_rows": [[8 * r - phase[1], 8 * r - phase[1] + 7] for r in rows], "wave_columns": [min(wx for wx, _, _ in waves), max(wx for wx, _, _ in waves)] if waves else []}))


if __name__ == "__main__":
    main()
