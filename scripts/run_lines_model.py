#!/usr/bin/env python3
"""Cache lines and 16-byte chunks a wave's run-brick gathers touch, under the two run layouts (CPU model, numpy).

The five benchmark poses that read run copies (view 1 and views 4-7 of the 8-view cycle, 1024^3 u8 at 2048x2048, full march) are
marched with the product's own ray set-up (View::get_ray, slab intersection, coordinate = k * A + B), its wave shapes and lane
maps (vr_march.h lane_pixel; vr_hip_api.cpp choose_tile_mapping / launch_frame) and its copy choice (runs across the march;
`dual_choice_bits` per 8x8-tile block on the oblique orthogonal view).  Per march step of a sample of workgroup tiles it counts, for

  run9: the resident layout — 9-element runs of 36 bytes, 2304-byte bricks of 8 cells along the run axis;
  run7: the aligned layout — 8-element runs of 32 bytes covering SEVEN cells, 2048-byte bricks (one 128-byte line = one 2x2 block
        of cell columns);

  lines/gather   distinct 128-byte lines the 64 slice-pair reads (8 bytes each) of a wave touch;
  chunks/gather  distinct 16-byte chunks per lane quad (4 consecutive lanes), summed over the wave's 16 quads;
  wg lines/8     distinct lines a workgroup (8 waves) touches over 8 consecutive steps — a proxy for the bytes it pulls.

Only lanes inside their ray segment count.  Simplifications: double precision instead of the kernel's fp32 (cell boundaries move by
rounding noise only), tile phase 0, the block-centre probe of dual_choice_bits only (a block whose centre ray misses keeps the frame's
default copy), a regular sample of tiles and of 8-step windows instead of the whole frame.

  python scripts/run_lines_model.py [--tiles 12] [--out profiles/run7_lines_model.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE, CHUNK = 128, 16
VIEWS = (1, 4, 5, 6, 7)
LANE_ROWS, LANE_COLUMNS, LANE_BLOCKS = 0, 1, 2


# ---- the two layouts: byte offset of the slice pair of cell (x, o, r) — x and o the column axes, r the run axis ------------------
def morton_column(lx, lo):
    """cell column (x & 7, o & 7) inside a brick: 2-D Morton order (vr_device.h run_cell_spread)"""
    lx, lo = np.asarray(lx), np.asarray(lo)
    return ((lx & 1) | ((lo & 1) << 1) | ((lx & 2) << 1) | ((lo & 2) << 2) | ((lx & 4) << 2) | ((lo & 4) << 3))


def run_offset(flavour, nbx, nbo, x, o, r):
    """flavour 9: kRunLen 9, 8 cells per brick along the run axis; flavour 7: 8 elements, 7 cells.  The read is 8 bytes from here."""
    x, o, r = np.asarray(x, np.int64), np.asarray(o, np.int64), np.asarray(r, np.int64)
    cells, run_bytes = (8, 36) if flavour == 9 else (7, 32)
    brick = ((r // cells) * nbo + (o >> 3)) * nbx + (x >> 3)
    return brick * (64 * run_bytes) + morton_column(x & 7, o & 7) * run_bytes + (r % cells) * 4


def units_of(offset, unit):
    """the one or two aligned units of `unit` bytes an 8-byte read at `offset` touches, shape (..., 2)"""
    return np.stack((offset // unit, (offset + 7) // unit), axis=-1)


def distinct(a, valid):
    """number of distinct values along the last axis among the entries whose `valid` is set"""
    a = np.where(valid, a, -1)
    a = np.sort(a, axis=-1)
    n = 1 + np.count_nonzero(a[..., 1:] != a[..., :-1], axis=-1)
    return n - (a[..., 0] == -1)


# ---- the product's frame policy for these poses ----------------------------------------------------------------------------------
def view_policy(v, half):
    d = np.abs(np.array(v.direction) * half)
    major = 2 if d[2] >= d[0] and d[2] >= d[1] else (1 if d[1] >= d[0] else 0)
    along = d.max() > 0.98 * np.sqrt((d * d).sum())
    run_y = major == 2                                            # runs across the march, never along it
    lane = LANE_BLOCKS if along else LANE_ROWS
    if not along:
        sx, sy = np.array(v.right_plane) * half, np.array(v.up_plane) * half
        if abs(sy[2]) * np.linalg.norm(sx) < abs(sx[2]) * np.linalg.norm(sy):
            lane = LANE_COLUMNS
    shape = 0
    if v.perspective and along:
        axis = 1 if run_y else 2
        shape = 2 if abs(v.up_plane[axis]) > abs(v.right_plane[axis]) else 1
    return dict(major=major, along=along, run_y=run_y, lane=lane, shape=shape, dual=(not v.perspective) and (not along))


def lane_pixels(lane_map, shape):
    """(8 waves, 64 lanes) -> pixel offsets inside the 32x16 workgroup tile (vr_march.h lane_pixel)"""
    lane = np.arange(64)
    qd, gu, gv = lane >> 4, lane & 3, (lane >> 2) & 3
    if lane_map == LANE_BLOCKS:
        gu, gv = ((lane >> 1) & 2) | (lane & 1), ((lane >> 2) & 2) | ((lane >> 1) & 1)
    elif lane_map == LANE_COLUMNS:
        gu, gv = gv, gu
    wave = np.arange(8)[:, None]
    if shape == 1:
        wx, wy, ox, oy = qd * 4 + gu, gv, (wave & 1) * 16, (wave >> 1) * 4
    elif shape == 2:
        wx, wy, ox, oy = gu, qd * 4 + gv, wave * 4, 0 * wave
    else:
        wx, wy, ox, oy = (qd & 1) * 4 + gu, (qd >> 1) * 4 + gv, (wave & 3) * 8, (wave >> 2) * 8
    return ox + wx, oy + wy


def rays(v, gx, gy):
    fx, fy = gx - v.width // 2, gy - v.height // 2
    o, d, r, u = (np.array(t, np.float64) for t in (v.origin, v.direction, v.right_plane, v.up_plane))
    if v.perspective:
        origin = np.broadcast_to(o, fx.shape + (3,))
        direction = d + r * fx[..., None] + u * fy[..., None]
    else:
        origin = o + r * fx[..., None] + u * fy[..., None]
        direction = np.broadcast_to(d, fx.shape + (3,))
    dd = np.where(direction == 0.0, 1e-5, direction)
    k1, k2 = (-1.0 - origin) / dd, (1.0 - origin) / dd
    k_in, k_out = np.minimum(k1, k2), np.maximum(k1, k2)
    kx, ky = np.maximum(k_in.max(-1), 0.0), k_out.min(-1)
    face = np.where((k_in[..., 2] >= k_in[..., 0]) & (k_in[..., 2] >= k_in[..., 1]), 2, np.where(k_in[..., 1] >= k_in[..., 0], 1, 0))
    return origin, direction, kx, ky, (kx < ky) & (ky > 0), face


def model_view(vr, index, n, size, step, tiles_side, window_stride):
    v = vr.benchmark_view(size, size, index)
    half = 0.5 * n
    pol = view_policy(v, half)
    px, py = lane_pixels(pol["lane"], pol["shape"])
    tiles_x, tiles_y = size // 32, size // 16
    tx = np.linspace(0, tiles_x - 1, tiles_side).astype(int)
    ty = np.linspace(0, tiles_y - 1, tiles_side).astype(int)
    nb = (n + 7) // 8
    out = {f: dict(lines=0.0, chunks=0.0, gathers=0, wg=0.0, windows=0) for f in (9, 7)}
    for tile_y in ty:
        for tile_x in tx:
            gx, gy = tile_x * 32 + px, tile_y * 16 + py
            origin, direction, kx, ky, alive, _ = rays(v, gx, gy)
            if not alive.any():
                continue
            along_y = pol["run_y"]
            if pol["dual"]:                                       # the block-centre probe of dual_choice_bits
                cx, cy = np.array([((tile_x // 8) * 8 + 4) * 32.0]), np.array([((tile_y // 8) * 8 + 4) * 16.0])
                _, _, _, _, hit, face = rays(v, cx.astype(int), cy.astype(int))
                if hit[0]:
                    along_y = face[0] != 1
            A, B = direction * half, origin * half + (half - 0.5)
            steps_max = int(np.ceil(((ky - kx) * alive).max() / step)) + 1
            starts = np.arange(0, max(steps_max - 8, 1), window_stride)
            s = (starts[:, None] + np.arange(8)).reshape(-1)                              # windows of 8 consecutive steps
            k = kx[..., None] + s * step                                                   # (8, 64, S)
            live = alive[..., None] & (k <= ky[..., None])
            cell = np.clip(np.floor(k[..., None] * A[:, :, None, :] + B[:, :, None, :]), 0, n - 1).astype(np.int64)
            x, y, z = cell[..., 0], cell[..., 1], cell[..., 2]
            o, r = (z, y) if along_y else (y, z)
            for f in (9, 7):
                off = run_offset(f, nb, nb, x, o, r)                                      # (8 waves, 64 lanes, S)
                lines = np.moveaxis(units_of(off, LINE), 1, 2)                            # (8, S, 64, 2)
                lv = np.moveaxis(np.repeat(live[..., None], 2, -1), 1, 2)
                per_gather = distinct(lines.reshape(8, len(s), 128), lv.reshape(8, len(s), 128))
                active = lv.reshape(8, len(s), 128).any(-1)
                chunks = np.moveaxis(units_of(off, CHUNK), 1, 2).reshape(8, len(s), 16, 8)
                per_quad = distinct(chunks, lv.reshape(8, len(s), 16, 8))
                acc = out[f]
                acc["lines"] += per_gather[active].sum(); acc["chunks"] += per_quad.sum(-1)[active].sum(); acc["gathers"] += int(active.sum())
                wg = np.moveaxis(lines, 1, 0).reshape(len(starts), 8, 8, 128)            # (window, step in window, wave, 64 x 2)
                wl = np.moveaxis(lv, 1, 0).reshape(len(starts), 8, 8, 128)
                per_window = distinct(wg.reshape(len(starts), -1), wl.reshape(len(starts), -1))
                busy = wl.reshape(len(starts), -1).any(-1)
                acc["wg"] += per_window[busy].sum(); acc["windows"] += int(busy.sum())
    return pol, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=12, help="sampled workgroup tiles per screen direction")
    ap.add_argument("--stride", type=int, default=96, help="march steps between the sampled 8-step windows")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run7_lines_model.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    vr = importlib.import_module("volume-rendering_amd")
    scene = vr.Scene().set_volume(dims=(a.n,) * 3, minmax=np.zeros((32 * 32 * 32, 2), np.uint8))
    step = float(scene.params.ray_step)
    rows = [f"run-brick line model: {a.n}^3 u8 at {a.size}x{a.size}, ray_step {step:.6g}, {a.tiles}x{a.tiles} sampled tiles, 8-step windows every {a.stride} steps",
            "run9 = 36-byte runs / 2304-byte bricks (8 cells), run7 = 32-byte runs / 2048-byte bricks (7 cells); scripts/run_lines_model.py",
            "",
            f"{'view':>4} {'copy':>9} {'wave':>5} {'lanes':>7} | {'lines/gather':>23} | {'chunks/gather':>23} | {'wg lines/8 steps':>25}",
            f"{'':>4} {'':>9} {'':>5} {'':>7} | {'run9':>7} {'run7':>7} {'':>7} | {'run9':>7} {'run7':>7} {'':>7} | {'run9':>8} {'run7':>8} {'':>7}"]
    passed = 0
    for index in VIEWS:
        pol, out = model_view(vr, index, a.n, a.size, step, a.tiles, a.stride)
        m = {f: (out[f]["lines"] / out[f]["gathers"], out[f]["chunks"] / out[f]["gathers"], out[f]["wg"] / out[f]["windows"]) for f in (9, 7)}
        change = [100.0 * (m[7][i] / m[9][i] - 1.0) for i in range(3)]
        passed += change[0] <= -10.0
        copy = "z|y/block" if pol["dual"] else ("along y" if pol["run_y"] else "along z")
        rows.append(f"{index:>4} {copy:>9} {('8x8', '16x4', '4x16')[pol['shape']]:>5} {('rows', 'columns', 'blocks')[pol['lane']]:>7} | "
                    f"{m[9][0]:7.2f} {m[7][0]:7.2f} {change[0]:+6.1f}% | {m[9][1]:7.2f} {m[7][1]:7.2f} {change[1]:+6.1f}% | {m[9][2]:8.1f} {m[7][2]:8.1f} {change[2]:+6.1f}%")
    rows += ["", f"gate (lines per wave-gather fall by at least 10 % on at least four of the five views): {passed} of {len(VIEWS)} -> {'PASS' if passed >= 4 else 'FAIL'}"]
    text = "\n".join(rows) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
