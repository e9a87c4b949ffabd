"""CPU tier of the shaded isosurface with depth (include/vr_hip.h vr_hip_render_iso): iso_render of tests/feature_ref.c — the frames and depths the GPU
tier expects — held against what is already pinned (mip_render's per-pixel maximum), against its own skipping emulation, and against
analytic ground truth, without a GPU; and the register figures of the built iso_kernel instantiations."""
import os
import re

import numpy as np
import pytest

from iso_helpers import NO_SURFACE, PAIRS, IsoRef, all_volumes, depth_bits, frame_params, views_for
from mip_helpers import MipRef, ramp_tf

SMALL_CASES = (32, 34, 36, 38, 40, 45)        # the golden cases tests/test_mip_model.py uses: no ESL, at most 120 x 96 pixels
LEVELS = (30.5, 100.0, 200.0)


def _case(golden, cid):
    return next(c for c in golden.cases() if c["id"] == cid)


def _params(golden, case, sampling):
    p = golden.params(case, sampling)
    p.esl, p.ray_threshold, p.light_kd = 0, 1.0, 0.0
    return p


@pytest.mark.parametrize("sampling", (1, 2), ids=("fp32", "q8"))
def test_hit_mask_is_where_the_mip_maximum_reaches_the_level(golden, sampling):
    """A ray has a first sample >= level exactly when its largest sample is >= level: mip_render's per-pixel maximum is pinned
    against the unmodified oracle by tests/test_mip_model.py.  The mask does not depend on `refine`."""
    tf = ramp_tf()
    hits = 0
    for cid in SMALL_CASES:
        case = _case(golden, cid)
        vox = np.ascontiguousarray(golden.voxels(case["volume"]))
        p = _params(golden, case, sampling)
        _, raw = MipRef.instance().render(p, vox, tf)
        missed = raw == 0xffffffff
        maximum = np.where(missed, np.float32(-1), raw.view(np.float32))
        scale = 1.0 if vox.dtype.itemsize == 1 else 257.0
        for level in LEVELS:
            want = ~missed & (maximum >= np.float32(level * scale))
            for refine in (0, 4):
                frame, depth, counters = IsoRef.instance().render(p, vox, tf, level * scale, refine)
                assert np.array_equal(depth >= 0, want), (cid, level, refine)
                assert np.array_equal(frame[..., 3] != 0, want), (cid, level, refine)      # the ramp's alpha is never 0
                assert np.array_equal(depth[~want], np.full(int((~want).sum()), -1, np.float32))
                assert counters["hits"] == int(want.sum())
            hits += int(want.sum())
    assert hits > 10000, hits


def test_skipping_emulation_changes_no_byte(vr, golden, oracle):
    """The restatement that skips the fetch of every march sample whose widened dilated bound is below the level — what the kernel may do
    with esl on — against the restatement that fetches them all: RGBA bytes and depth bits, on every (volume, level) pair of the GPU
    tier, both samplings, nine views; and skipping does skip."""
    ref, tf, volumes = IsoRef.instance(), ramp_tf(), all_volumes(golden)
    skipped = {}
    for name, level in PAIRS:
        vox = volumes[name]
        samples = fetches = hits = 0
        for label, view in views_for(vr, golden, name):
            for sampling in (1, 2):
                p = frame_params(vr, oracle, vox, view, sampling, 0)
                plain, plain_depth, c0 = ref.render(p, vox, tf, level, 4)
                skip, skip_depth, c1 = ref.render(p, vox, tf, level, 4, skipping=True)
                assert np.array_equal(plain, skip), (name, level, label, sampling)
                assert np.array_equal(depth_bits(plain_depth), depth_bits(skip_depth)), (name, level, label, sampling)
                assert c0["samples"] == c1["samples"] and c0["hits"] == c1["hits"] and c0["fetches"] >= c1["fetches"]
                samples += c0["fetches"]
                fetches += c1["fetches"]
                hits += c0["hits"]
        skipped[(name, level)] = 1.0 - fetches / max(samples, 1)
        print(f"{name} @ {level}: {hits} hits, {100 * skipped[(name, level)]:.1f} % of the march fetches skipped")
        assert (hits == 0) == ((name, level) in NO_SURFACE), (name, level, hits)
    assert skipped[("zeros", 24.5)] == 1.0                    # every fetch
    assert skipped[("late_max", 200.0)] > 0.5 and skipped[("corner", 24.5)] > 0.5
    assert skipped[("blob_40x24x56", 200.0)] > 0.2


def _rays(p):
    """origin, direction, kx of every pixel of the whole frame in the fp32 operations of View::get_ray and Raycaster::intersect"""
    f = np.float32
    v = p.view
    ys, xs = np.mgrid[0:v.height, 0:v.width]
    fx = (xs - int(v.width // 2)).astype(f)
    fy = (ys - int(v.height // 2)).astype(f)
    vo, vd, vr_, vu = (np.array(list(a), f) for a in (v.origin, v.direction, v.right_plane, v.up_plane))
    shape = fx.shape + (3,)
    if v.perspective:
        o = np.broadcast_to(vo, shape).astype(f)
        d = ((vd + vr_ * fx[..., None]).astype(f) + (vu * fy[..., None]).astype(f)).astype(f)
    else:
        d = np.broadcast_to(vd, shape).astype(f)
        o = ((vo + vr_ * fx[..., None]).astype(f) + (vu * fy[..., None]).astype(f)).astype(f)
    dd = np.where(d == 0, f(0.00001), d).astype(f)
    k1 = ((f(-1) - o) / dd).astype(f)
    k2 = ((f(1) - o) / dd).astype(f)
    kx = np.maximum(np.minimum(k1, k2).max(axis=-1), f(0)).astype(f)
    return o, d, kx


def test_refinement_only_moves_the_hit_towards_the_eye(vr, golden, oracle):
    """hi never grows with `refine`; refine = 0 leaves the depth on a member of the ray's own k sequence (kx, kx + step, ... by repeated
    fp32 addition)."""
    ref, tf, volumes = IsoRef.instance(), ramp_tf(), all_volumes(golden)
    checked = 0
    for name, level, views in (("bucky", 100.0, (1, 5)), ("late_max", 24.5, (2, 6))):
        vox = volumes[name]
        for i in views:
            p = frame_params(vr, oracle, vox, vr.benchmark_view(80, 80, i), 1, 0)
            depths = [ref.render(p, vox, tf, level, r)[1] for r in (0, 1, 2, 4, 8, 16)]
            hit = depths[0] >= 0
            assert hit.sum() > 500
            for a, b in zip(depths, depths[1:]):
                assert np.array_equal(b >= 0, hit) and (b[hit] <= a[hit]).all(), (name, i)
            assert (depths[-1][hit] < depths[0][hit]).any()
            _, _, k = _rays(p)
            member = np.zeros_like(hit)
            step = np.float32(p.ray_step)
            for _ in range(int(4.0 / p.ray_step) + 2):
                member |= k == depths[0]
                k = (k + step).astype(np.float32)
            assert member[hit].all(), (name, i, int((~member[hit]).sum()))
            checked += int(hit.sum())
    assert checked > 2000


def _sphere(dtype):
    """64^3: clip(rint(128 + (20 - r) * 8)), r the distance in voxels from a centre 1.3 / -0.7 / 0.4 off the middle: a ramp of 8 grey levels
    per voxel through the value 128 at r = 20"""
    z, y, x = np.mgrid[0:64, 0:64, 0:64].astype(np.float64)
    centre = np.array([31.5 + 1.3, 31.5 - 0.7, 31.5 + 0.4])
    r = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    v = np.clip(np.rint(128 + (20 - r) * 8), 0, 255).astype(np.uint8)
    return (v if dtype == np.uint8 else v.astype(np.uint16) * 257), centre


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=("u8", "u16"))
def test_analytic_sphere(vr, oracle, dtype):
    """The definition against ground truth it was not derived from.  Level 128 (x 257 for 2-byte voxels), refine 8, light_kd 1:
     * every hit lies within 0.125 voxels of the sphere of radius 20 — one grey level is 1/8 voxel: +-1/2 level of quantisation is
       0.0625, the interpolation's curvature term h^2 / 8R is 0.006, the bisection interval ray_step * N/2 / 2^8 is 0.004;
     * the shading factor recovered from the frame (lit byte / unlit byte of the largest channel; the unlit byte is 65, so one byte is
       0.015) is within 0.1 of the analytic |n . l|: the 8-bit field's gradient noise, a quantisation step of 1 in a central difference of 16."""
    vox, centre = _sphere(dtype)
    level = 128.0 * (1 if dtype == np.uint8 else 257)
    tf, ref = ramp_tf(), IsoRef.instance()
    for i in (0, 1, 4, 5):
        view = vr.benchmark_view(96, 96, i)
        p = frame_params(vr, oracle, vox, view, 1, 0, light_kd=1.0)
        lit, depth, _ = ref.render(p, vox, tf, level, 8)
        p_unlit = frame_params(vr, oracle, vox, view, 1, 0, light_kd=0.0)
        unlit, depth_unlit, _ = ref.render(p_unlit, vox, tf, level, 8)
        assert np.array_equal(depth_bits(depth), depth_bits(depth_unlit))
        hit = depth >= 0
        assert hit.sum() > 1000, (i, int(hit.sum()))
        o, d, _ = _rays(p)
        pos = o.astype(np.float64) + d.astype(np.float64) * depth[..., None].astype(np.float64)
        texel = pos * 32.0 + 31.5
        off = texel[hit] - centre
        r = np.sqrt((off ** 2).sum(axis=-1))
        print(f"view {i}: {int(hit.sum())} hits, |r - 20| max {np.abs(r - 20).max():.4f}")
        assert np.abs(r - 20).max() <= 0.125, (i, float(np.abs(r - 20).max()))
        channel = int(np.argmax(unlit[hit][0, :3]))
        base = unlit[hit][:, channel].astype(np.float64)
        assert (base == 65).all()
        recovered = lit[hit][:, channel].astype(np.float64) / base
        n = off / r[:, None]
        l = np.array(list(view.light_pos), np.float64) - pos[hit]
        l /= np.sqrt((l ** 2).sum(axis=-1))[:, None]
        analytic = np.abs((n * l).sum(axis=-1))
        err = np.abs(recovered - analytic)
        print(f"view {i}: shading error max {err.max():.4f} mean {err.mean():.4f}")
        assert err.max() <= 0.1, (i, float(err.max()))
        assert (lit[hit][:, 3] == unlit[hit][:, 3]).all()          # alpha is not shaded


def test_iso_kernels_do_not_spill(vr):
    """Every iso_kernel instantiation of the build (its resource log): no scratch, no SGPR or VGPR spilled, and within the 80 SGPRs and
    64 VGPRs of 8 waves per SIMD — all of them, the index-arithmetic ones included (DESIGN.md section 4.5 has the figures)."""
    import subprocess
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    log = os.path.join(csrc, "resource_usage.log")
    if not os.path.exists(log):
        subprocess.check_call(["make", "-B", "-C", csrc])
    found = {}
    for m in re.finditer(r"Function Name: (\S*iso_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)E\S*).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", open(log).read(), flags=re.S):
        sampling, bpv, addr, layout, sgprs, vgprs, scratch, sspill, vspill = (int(g) for g in m.groups()[1:])
        found[(sampling, bpv, addr, layout)] = m.group(1)
        assert scratch == 0 and sspill == 0 and vspill == 0, (m.group(1), scratch, sspill, vspill)
        assert sgprs <= 80 and vgprs <= 64, (m.group(1), sgprs, vgprs)
    # {TRILINEAR, Q8} x ({u8, u16} x (quad bricks x 3 addressing paths + linear x 2) + u16 oct bricks x 2) = 24
    assert len(found) == 24, sorted(found)
    assert {k[0] for k in found} == {1, 2}
    assert not [k for k in found if k[3] in (2, 3, 4, 6, 7, 8)], "an isosurface frame never reads the run bricks, the voxel bricks or the column windows"
