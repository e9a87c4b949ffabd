"""The float64 model tier's reference: a plain, vectorised numpy statement of the feature frames of include/vr_hip.h — the MIP, the section
frames, the depth frames and picks, and the labelled, tf2d and fused composites — written from the header's paragraphs and DESIGN.md, in
double precision.  It is a SECOND READING: nothing here is taken from tests/*_ref.c, nothing imports their helpers, and the only texts it
shares with the restatements are the two conventions of oracle/vr_oracle.c it was told to share: View::get_ray / Raycaster::intersect, and
the texel map  texel = k * A + B  with  A = dir * N/2,  B = origin * N/2 + N/2 - 1/2  ("voxel i's centre is at texel i").

What is kept is what the contract defines as SEMANTICS: the sample sequence `k = kx; while (k <= ky) k += ray_step`, the _Q8 weights
rint(w * 256) / 256, the `c.w > 0.05` dense test, the clamps, and map_float_int for the final bytes.  What is dropped is everything that
is ROUNDING: no fma, no fp32 intermediates, no Newton reciprocal square root (np.sqrt), products and sums in the order they are read.
`dtype=np.float32` evaluates the same statements in single precision.  That evaluation is never compared with the product: the distance
between the two evaluations is the rounding noise any correct fp32 implementation carries, which is where the tier's tolerances come
from, and a pixel whose discrete record differs between them sits on a decision no fp32 implementation is bound to take one way.

Covered: orthogonal and perspective views, whole frames only (x0 = 0, one band), the clip contract's steps 1-3, TRILINEAR and _Q8, the
reference's cue (light_kd), early termination, esl = 0.  Not covered (each has an anchor of its own): leaping, NEAREST,
the shadow grid, gradient lighting, pre-integration, the isosurface, backdrop and hybrid frames.  The hooks run unlit, unshadowed and point
classified; depth frames are point classified only.

Arrays are per pixel, flattened row-major (y up, as the frame is stored): index y * width + x.  Per-sample records are (samples, pixels)."""
import numpy as np

TF_SIZE = 128
DENSE = 0.05                                            # the composite's `c.w > 0.05f`
CUE_MIN_KD = 0.01                                       # ... and its `light_kd > 0.01f`
CUE_OFFSET = 0.01                                       # the cue's second sample lies 0.01 model units towards the light
ZERO_DIR = float(np.float32(0.00001))                   # what intersect puts in place of an exact zero of the direction
MAX_SAMPLES = 4096
SECTION_MODES = ("point", "max", "min", "mean")
DEPTH_MODES = ("first", "peak", "mean")


def _vec(a, T):
    return np.array([a[0], a[1], a[2]], dtype=T)


def full_scale(vox):
    return 255.0 if vox.dtype.itemsize == 1 else 65535.0


def write_color(c):
    """map_float_int(f, 256) per channel: truncation toward zero of f * 256, clamped to 0..255"""
    q = np.trunc(np.nan_to_num(np.asarray(c, np.float64) * 256.0, nan=0.0, posinf=255.0, neginf=0.0))
    return np.clip(q, 0, 255).astype(np.uint8)


# ---- rays -------------------------------------------------------------------------------------------------------------------------------

class Rays:
    """origin o and direction d (pixels, 3), the segment kx, ky and the hit flag of every pixel of a whole frame, after get_ray, intersect
    and — where a clip is given — steps 1-3 of the clip contract"""

    def __init__(self, o, d, kx, ky, hit, width, height, T):
        self.o, self.d, self.kx, self.ky, self.hit, self.width, self.height, self.T = o, d, kx, ky, hit, width, height, T

    def frame(self, a):
        return a.reshape((self.height, self.width) + a.shape[1:])


def rays(p, clip=None, dtype=np.float64):
    """clip: (box_min, box_max, plane) with None for a missing member, as vr_clip has them; None = no clip (the identity clip changes no bit)"""
    T = np.dtype(dtype).type
    v = p.view
    W, H = int(v.width), int(v.height)
    assert p.x0 == 0 and p.out_width == W and p.out_rows == H and p.band_stride == 1 and p.band_first == 0 and p.band_rows >= H, "whole frames only"
    ys, xs = np.mgrid[0:H, 0:W]
    fx = (xs.reshape(-1, 1) - W // 2).astype(T)
    fy = (ys.reshape(-1, 1) - H // 2).astype(T)
    vo, vd, vr, vu = (_vec(a, T) for a in (v.origin, v.direction, v.right_plane, v.up_plane))
    if v.perspective:
        o = np.broadcast_to(vo, (W * H, 3)).copy()
        d = (vd + vr * fx) + vu * fy
    else:
        d = np.broadcast_to(vd, (W * H, 3)).copy()
        o = (vo + vr * fx) + vu * fy
    dd = np.where(d == 0, T(ZERO_DIR), d)
    k1, k2 = (T(-1) - o) / dd, (T(1) - o) / dd
    kx = np.maximum(np.minimum(k1, k2).max(axis=1), T(0))
    ky = np.maximum(k1, k2).min(axis=1)
    hit = (kx < ky) & (ky > 0)
    if clip is not None:
        box_min, box_max, plane = clip
        if box_min is not None or box_max is not None:
            lo = _vec(box_min or (-1.0, -1.0, -1.0), T)
            hi = _vec(box_max or (1.0, 1.0, 1.0), T)
            k1, k2 = (lo - o) / dd, (hi - o) / dd
            kx = np.maximum(kx, np.minimum(k1, k2).max(axis=1))
            ky = np.minimum(ky, np.maximum(k1, k2).min(axis=1))
        if plane is not None and any(float(c) != 0.0 for c in plane):
            n, dist = _vec(plane, T), T(np.float32(plane[3]))
            dn, on = (d * n).sum(axis=1), (o * n).sum(axis=1) + dist
            with np.errstate(divide="ignore", invalid="ignore"):
                kp = -on / dn
            kx = np.where(dn > 0, np.maximum(kx, kp), kx)
            ky = np.where(dn < 0, np.minimum(ky, kp), ky)
            hit = hit & np.where(dn == 0, on >= 0, True)
        hit = hit & (kx < ky) & (ky > 0)
    return Rays(o, d, kx, ky, hit, W, H, T)


def texel_map(r, vox):
    """A, B (pixels, 3) of  texel = k * A + B  for the volume's dims: half = N / 2 per axis"""
    z, y, x = vox.shape
    half = np.array([x, y, z], dtype=r.T) * r.T(0.5)
    return r.d * half, r.o * half + half - r.T(0.5), half


# ---- the field --------------------------------------------------------------------------------------------------------------------------

def _axis(c, n, q8):
    fl = np.floor(c)
    w = c - fl
    if q8:
        w = np.rint(w * 256) / 256
    i = np.clip(fl, -1, n).astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), w.astype(c.dtype)


def field(vox, xb, yb, zb, q8=False):
    """the trilinearly interpolated RAW value at texel coordinates (xb, yb, zb), clamp addressing; q8: weights rounded to 8 fractional bits"""
    T = xb.dtype.type
    z, y, x = vox.shape
    x0, x1, wx = _axis(xb, x, q8)
    y0, y1, wy = _axis(yb, y, q8)
    z0, z1, wz = _axis(zb, z, q8)

    def along_x(zi, yi):
        a, b = vox[zi, yi, x0].astype(T), vox[zi, yi, x1].astype(T)
        return a + wx * (b - a)

    def along_y(zi):
        a, b = along_x(zi, y0), along_x(zi, y1)
        return a + wy * (b - a)
    a, b = along_y(z0), along_y(z1)
    return a + wz * (b - a)


def gradient(vox, xb, yb, zb, half, q8=False):
    """step 1 of the lighting contract: central differences one texel apart of the interpolated value, times half_x / y / z"""
    one = xb.dtype.type(1)
    gx = (field(vox, xb + one, yb, zb, q8) - field(vox, xb - one, yb, zb, q8)) * half[0]
    gy = (field(vox, xb, yb + one, zb, q8) - field(vox, xb, yb - one, zb, q8)) * half[1]
    gz = (field(vox, xb, yb, zb + one, q8) - field(vox, xb, yb, zb - one, q8)) * half[2]
    return gx, gy, gz


def tf_coordinate(raw, scale_to):
    """tb: raw / full scale * 128 - 1/2, clamped to [0, 127]"""
    T = raw.dtype.type
    return np.clip(raw * (T(TF_SIZE) / T(scale_to)) - T(0.5), T(0), T(TF_SIZE - 1))


def tf_weights(tb, q8):
    i = np.floor(tb).astype(np.int64)
    w = tb - i.astype(tb.dtype)
    if q8:
        w = (np.rint(w * 256) / 256).astype(tb.dtype)
    return i, np.minimum(i + 1, TF_SIZE - 1), w


def tf(table, raw, scale_to, q8=False):
    """the filtered 128-entry lookup of a raw value: (..., 4)"""
    t = np.asarray(table).reshape(TF_SIZE, 4).astype(raw.dtype)
    i, i1, w = tf_weights(tf_coordinate(raw, scale_to), q8)
    return t[i] + w[..., None] * (t[i1] - t[i])


# ---- the sample sequence ---------------------------------------------------------------------------------------------------------------------

def sequence(kx, ky, step, active):
    """K (samples, pixels): k = kx, then k += step by repeated addition in the model's precision; M: the samples with k <= ky of the active pixels"""
    T = kx.dtype.type
    step = T(np.float32(step))
    assert step > 0
    span = np.where(active, ky - kx, T(0))
    S = int(np.floor(span.max() / step)) + 2 if active.any() else 1
    assert S <= MAX_SAMPLES, S
    inc = np.full((S, kx.shape[0]), step, dtype=T)
    inc[0] = np.where(active, kx, T(0))
    K = np.cumsum(inc, axis=0, dtype=T)
    return K, active[None, :] & (K <= np.where(active, ky, T(-1))[None, :])


class March:
    """the samples of every ray of a frame on the segments [kx, ky] of the active pixels: K, M, the texel coordinates and the raw values"""

    def __init__(self, r, vox, step, q8, kx=None, ky=None, active=None, single=False):
        self.r, self.vox, self.q8, self.T = r, vox, q8, r.T
        kx, ky, active = (r.kx if kx is None else kx), (r.ky if ky is None else ky), (r.hit if active is None else active)
        if single:                                      # POINT: the one sample at kx == ky
            self.K, self.M = np.where(active, kx, r.T(0))[None, :], active[None, :].copy()
        else:
            self.K, self.M = sequence(kx, ky, step, active)
        self.A, self.B, self.half = texel_map(r, vox)
        self.X = tuple(self.K * self.A[:, j] + self.B[:, j] for j in range(3))
        self.raw = field(vox, *self.X, q8)
        self.count = self.M.sum(axis=0)


# ---- projections -----------------------------------------------------------------------------------------------------------------------------

def mip(p, vox, table, clip=None, dtype=np.float64):
    """vr_hip_render_mip, TRILINEAR / _Q8, esl = 0: value = the maximum of the samples, starting at 0"""
    q8 = int(p.sampling) == 2
    r = rays(p, clip, dtype)
    m = March(r, vox, p.ray_step, q8)
    value = np.where(m.M, m.raw, r.T(0)).max(axis=0)
    colour = np.where(r.hit[:, None], tf(table, value, full_scale(vox), q8), r.T(0))
    return dict(hit=r.hit, count=m.count, value=value, colour=colour, rgba=write_color(colour))


def section(p, vox, table, plane, half_width=0.0, mode="point", window=None, clip=None, dtype=np.float64):
    """vr_hip_render_section.  hit: the pixel carries a section; depth: kc (POINT) or the narrowed kx (thick modes), -1 elsewhere"""
    q8 = int(p.sampling) == 2
    r = rays(p, clip, dtype)
    T = r.T
    n, dist, h = _vec(plane, T), T(np.float32(plane[3])), T(np.float32(half_width))
    dn, on = (r.d * n).sum(axis=1), (r.o * n).sum(axis=1) + dist
    crossing = r.hit & (dn != 0)
    safe = np.where(dn != 0, dn, T(1))
    kc = -on / safe
    if mode == "point":
        hit = crossing & (r.kx <= kc) & (kc <= r.ky)
        m = March(r, vox, p.ray_step, q8, kc, kc, hit, single=True)
        front = kc
        value = m.raw[0]
    else:
        ka, kb = ((-h) - on) / safe, (h - on) / safe
        kx, ky = np.maximum(r.kx, np.minimum(ka, kb)), np.minimum(r.ky, np.maximum(ka, kb))
        hit = crossing & (kx < ky) & (ky > 0)
        m = March(r, vox, p.ray_step, q8, kx, ky, hit)
        front = kx
        if mode == "max":
            value = np.where(m.M, m.raw, T(0)).max(axis=0)
        elif mode == "min":
            value = np.where(m.M, m.raw, T(np.inf)).min(axis=0)
        else:
            assert mode == "mean", mode
            value = np.where(m.M, m.raw, T(0)).sum(axis=0) / np.maximum(m.count, 1).astype(T)
    value = np.where(hit, value, T(0))
    if window is None or (float(window[0]) == 0.0 and float(window[1]) == 0.0):
        colour = tf(table, value, full_scale(vox), q8)
    else:
        lo, hi = T(np.float32(window[0])), T(np.float32(window[1]))
        g = np.clip((value - lo) * (T(1) / (hi - lo)), T(0), T(1))
        colour = np.stack([g, g, g, np.ones_like(g)], axis=1)
    colour = np.where(hit[:, None], colour, T(0))
    return dict(hit=hit, count=np.where(hit, m.count, 0), value=value, depth=np.where(hit, front, T(-1)), colour=colour, rgba=write_color(colour))


def depth(p, vox, table, opacity, clip=None, dtype=np.float64):
    """vr_hip_render_depth, point classified, esl = 0: all three modes from one alpha-only march.  Returns {mode: dict(depth, value, index)},
    and alpha, count, hit (the ray has samples) shared by the modes.  index: the recorded sample (FIRST, PEAK), -1 where there is none."""
    q8 = int(p.sampling) == 2
    r = rays(p, clip, dtype)
    T = r.T
    m = March(r, vox, p.ray_step, q8)
    a = tf(table, m.raw, full_scale(vox), q8)[..., 3]
    P = r.hit.shape[0]
    thr, opacity = T(np.float32(p.ray_threshold)), T(np.float32(opacity))
    acc, alive, count = np.zeros(P, T), np.ones(P, bool), np.zeros(P, np.int64)
    first, peak = np.full(P, -1, np.int64), np.full(P, -1, np.int64)
    best, sg, sk, sv = np.zeros(P, T), np.zeros(P, T), np.zeros(P, T), np.zeros(P, T)
    for i in range(m.M.shape[0]):
        on = m.M[i] & alive
        if not on.any():
            if not m.M[i].any():
                break
            continue
        g = np.where(on, a[i] * (T(1) - acc), T(0))
        acc = acc + g
        count += on
        first = np.where(on & (first < 0) & (acc >= opacity), i, first)
        higher = on & (g > best)
        best, peak = np.where(higher, g, best), np.where(higher, i, peak)
        sg, sk, sv = sg + g, sk + m.K[i] * g, sv + m.raw[i] * g
        alive &= ~(on & (acc > thr))
    cols = np.arange(P)

    def recorded(index):
        at = np.maximum(index, 0)
        return dict(depth=np.where(index >= 0, m.K[at, cols], T(-1)), value=np.where(index >= 0, m.raw[at, cols], T(-1)), index=index)
    some = sg > 0
    by = np.where(some, sg, T(1))
    out = {"first": recorded(first), "peak": recorded(peak),
           "mean": dict(depth=np.where(some, sk / by, T(-1)), value=np.where(some, sv / by, T(-1)), index=np.where(some, 0, -1))}
    out.update(alpha=acc, count=count, hit=count > 0, rays=r, map=(m.A, m.B))
    return out


def pick(frame, mode, xy, voxel_offset=0.0):
    """vr_hip_pick from a depth() result: what the whole frame stores at the pixels xy, the position o + d * k and the continuous voxel
    index k * A + B.  voxel_offset: the tier's own mutation ("voxel i's centre is at i + 1/2"), 0 in the contract."""
    r, (A, B) = frame["rays"], frame["map"]
    T = r.T
    at = np.array([y * r.width + x for x, y in xy], np.int64)
    k = frame[mode]["depth"][at]
    hit = k >= 0
    kk = np.where(hit, k, T(0))[:, None]
    return dict(hit=hit, k=k, value=frame[mode]["value"][at], alpha=frame["alpha"][at],
                position=np.where(hit[:, None], r.o[at] + r.d[at] * kk, T(0)),
                voxel=np.where(hit[:, None], kk * A[at] + B[at] + T(voxel_offset), T(0)))


# ---- composites ------------------------------------------------------------------------------------------------------------------------------

def _cue(m, p, c, raw):
    """the reference's cue on the samples whose looked-up (or hooked) colour is dense: (raw_l - raw) / full scale * light_kd on the three colour
    channels, raw_l the field 0.01 model units towards view.light_pos.  Returns (colour, dense)."""
    T = m.T
    dense = m.M & (c[..., 3] > T(DENSE))
    if not float(np.float32(p.light_kd)) > CUE_MIN_KD:
        return c, dense
    lp = _vec(p.view.light_pos, T)
    pt = [m.r.o[:, j] + m.r.d[:, j] * m.K for j in range(3)]
    dl = [lp[j] - pt[j] for j in range(3)]
    length = np.sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2])
    safe = np.where(length > 0, length, T(1))
    raw_l = field(m.vox, *(m.X[j] + dl[j] / safe * T(CUE_OFFSET) * m.half[j] for j in range(3)), m.q8)
    diffuse = np.where(dense, (raw_l - raw) / T(full_scale(m.vox)) * T(np.float32(p.light_kd)), T(0))
    c = c.copy()
    c[..., :3] += diffuse[..., None]
    return c, dense


def _front_to_back(m, layers, threshold):
    """acc += c * (1 - acc.w) per layer and sample, front to back; `acc.w > ray_threshold` once per sample, behind every layer"""
    T = m.T
    P = m.M.shape[1]
    acc, alive, count = np.zeros((P, 4), T), np.ones(P, bool), np.zeros(P, np.int64)
    thr = T(np.float32(threshold))
    for i in range(m.M.shape[0]):
        on = m.M[i] & alive
        if not on.any():
            if not m.M[i].any():
                break
            continue
        for c in layers:
            acc = np.where(on[:, None], acc + c[i] * (T(1) - acc[:, 3])[:, None], acc)
        count += on
        alive &= ~(on & (acc[:, 3] > thr))
    used = m.M & (np.arange(m.M.shape[0])[:, None] < count[None, :])
    return acc, count, used


def _composite_result(m, acc, count, used, records):
    out = dict(hit=m.r.hit, count=count, acc=acc, rgba=write_color(acc), used=used)
    for name, a in records.items():
        out[name] = np.where(used, a, -1).astype(np.int16)      # (a flag, a label of 0..255, a row of 0..7; -1: the sample is not composited)
    return out


def composite(p, vox, table, clip=None, dtype=np.float64):
    """vr_hip_render, TRILINEAR / _Q8, esl = 0, with the reference's cue and early termination"""
    q8 = int(p.sampling) == 2
    m = March(rays(p, clip, dtype), vox, p.ray_step, q8)
    c, dense = _cue(m, p, tf(table, m.raw, full_scale(vox), q8), m.raw)
    return _composite_result(m, *_front_to_back(m, [c], p.ray_threshold), dict(dense=dense))


def labelled(p, vox, table, labels, entries, clip=None, dtype=np.float64):
    """vr_hip_render_labelled: behind the lookup and in front of the dense test, the table entry of the nearest voxel's label.
    entries: (256, 5) of { colour[3], mix, opacity }"""
    q8 = int(p.sampling) == 2
    m = March(rays(p, clip, dtype), vox, p.ray_step, q8)
    T = m.T
    c = tf(table, m.raw, full_scale(vox), q8)
    z, y, x = vox.shape
    ix, iy, iz = (np.floor(np.clip(m.X[j] + T(0.5), T(0), T(n - 1))).astype(np.int64) for j, n in enumerate((x, y, z)))
    label = np.asarray(labels)[iz, iy, ix].astype(np.int64)
    e = np.asarray(entries, np.float32).reshape(-1, 5).astype(T)[label]
    rgb = c[..., :3] + e[..., 3:4] * (e[..., :3] * c[..., 3:4] - c[..., :3])
    c = np.concatenate([rgb, c[..., 3:4]], axis=-1) * e[..., 4:5]
    c, dense = _cue(m, p, c, m.raw)
    return _composite_result(m, *_front_to_back(m, [c], p.ray_threshold), dict(dense=dense, label=label))


def gradient_row(g, g_scale, rows):
    """step 5 of the tf2d contract: (j, wg)"""
    T = g.dtype.type
    tg = np.clip(g * T(np.float32(g_scale)), T(0), T(rows - 1))
    j = np.minimum(np.floor(tg).astype(np.int64), rows - 2)
    return j, tg - j.astype(T)


def tf2d(p, vox, table2d, g_scale, clip=None, dtype=np.float64):
    """vr_hip_render_tf2d: the looked-up colour is the blend of two rows of the (rows, 128, 4) table, picked by the gradient's length"""
    q8 = int(p.sampling) == 2
    m = March(rays(p, clip, dtype), vox, p.ray_step, q8)
    T = m.T
    t = np.asarray(table2d).astype(T)
    rows = t.shape[0]
    i, i1, w = tf_weights(tf_coordinate(m.raw, full_scale(vox)), q8)
    gx, gy, gz = gradient(vox, *m.X, m.half, q8)
    g = np.sqrt(gx * gx + gy * gy + gz * gz)
    j, wg = gradient_row(g, g_scale, rows)
    lower = t[j, i] + w[..., None] * (t[j, i1] - t[j, i])
    upper = t[j + 1, i] + w[..., None] * (t[j + 1, i1] - t[j + 1, i])
    c = lower + wg[..., None] * (upper - lower)
    own = (t != t[0]).any(axis=(0, 2))                  # entries at which some row differs from row 0: only there does the row matter
    depends = own[i] | own[i1]
    c, dense = _cue(m, p, c, m.raw)
    out = _composite_result(m, *_front_to_back(m, [c], p.ray_threshold), dict(dense=dense, row=np.where(m.M & depends, j, -1)))
    out["g"] = g
    return out


def fused(p, vox, table, second, table_b, mode="sum", weight_a=1.0, weight_b=1.0, clip=None, dtype=np.float64):
    """vr_hip_render_fused: field A with its dense test and cue, times weight_a; field B at the same coordinates and weights, emissive, times
    weight_b; SUM: one accumulation of the sum, OVER: A in front of B within the sample, one termination test behind both"""
    q8 = int(p.sampling) == 2
    m = March(rays(p, clip, dtype), vox, p.ray_step, q8)
    T = m.T
    ca, dense = _cue(m, p, tf(table, m.raw, full_scale(vox), q8), m.raw)
    cb = tf(table_b, field(second, *m.X, q8), full_scale(second), q8)
    ca, cb = ca * T(np.float32(weight_a)), cb * T(np.float32(weight_b))
    layers = [ca + cb] if mode == "sum" else [ca, cb]
    assert mode in ("sum", "over"), mode
    return _composite_result(m, *_front_to_back(m, layers, p.ray_threshold), dict(dense=dense))
