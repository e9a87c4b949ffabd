"""The corner exchange of the voxel-window column march (voxcol_march, csrc/vr_kernels.hip): the four owners' aligned dwords are exchanged
once per CELL GROUP (the three cells base .. base + 2 whose four slices one dword holds) and the samples of the group pick their pair with a
v_perm selector chosen by sub - base; a lane's switch to its second column is made where the corners are exchanged.

CPU: a model of the selector logic against the per-sample alignbyte + perm formula it replaces, exhaustively.
GPU: the smallest frames in which the reuse can go wrong — march extents around the window and group edges, several samples per cell and one
cell per sample, both march directions on all three axes, flips between two samples of one cell (asserted by a CPU replay), a transfer
function whose holes begin and end groups at arbitrary cells — byte for byte against the CPU oracle, through voxcol_pairs_kernel (column copy
0), voxcol_tri_kernel (2) and colmarch_kernel (1), each asserted in the launch record; and the same frames once under the bounds-checked build."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_column_edges as edges
from gpu_feature import BOUNDS_LIB
from helpers import ColumnScene, axis_view, column_params, voxel_windows_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from lane_march_waves import mixed_entry_waves, pixel_segments  # noqa: E402

gpu_test = pytest.mark.gpu
BUFFER = 128
F = np.float32

# ---- the selector logic, on the CPU --------------------------------------------------------------------------------------------------

FIRST_STAGE, W0_SEL, W1_SEL = 0x05010400, 0x05040100, 0x07060302


def alignbyte(hi, lo, n):
    """v_alignbyte_b32: bytes n .. n + 3 of the eight bytes {hi, lo}"""
    return (((hi << 32) | lo) >> (8 * (n & 3))) & 0xFFFFFFFF


def perm(s0, s1, sel):
    """v_perm_b32 for selectors 0 .. 7: byte i of the result is byte sel[i] of the eight bytes {s0, s1}"""
    both, out = (s0 << 32) | s1, 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xFF
        assert s < 8, hex(sel)
        out |= ((both >> (8 * s)) & 0xFF) << (8 * i)
    return out


def owner_dword(window17, nxt3, at_cell):
    """the dword an owner aligns at cell `at_cell`: slices at_cell .. at_cell + 3 of its column (o.x .. o.w and nx of the kernel)"""
    data = bytes(window17) + bytes(nxt3)                                   # 16 slices of the window, the next window's first dword
    o = [int.from_bytes(data[4 * i:4 * i + 4], "little") for i in range(5)]
    qw = at_cell >> 2
    return alignbyte(o[qw + 1], o[qw], at_cell & 3)


def pair_per_sample(columns, sub):
    """today's formula: every sample aligns at its own cell; (w0, w1) of the columns (u,v) (u+1,v) (u,v+1) (u+1,v+1)"""
    p00, p10, p01, p11 = (owner_dword(w, n, sub) for w, n in columns)
    t0, t1 = perm(p10, p00, FIRST_STAGE), perm(p11, p01, FIRST_STAGE)
    return perm(t1, t0, W0_SEL), perm(t1, t0, W1_SEL)


def pair_from_group(held, base, sub):
    """the group's four dwords, aligned at `base`; the selector set of sub - base"""
    assert 0 <= sub - base <= 2
    sel = (FIRST_STAGE + (sub - base) * 0x01010101) & 0xFFFFFFFF
    t0, t1 = perm(held[1], held[0], sel), perm(held[3], held[2], sel)
    return perm(t1, t0, W0_SEL), perm(t1, t0, W1_SEL)


def group_base(forward, sub):
    """where a new group is aligned: at the sample's cell marching up, so that it ENDS there marching down (not below the window's first cell)"""
    return sub if forward else max(sub - 2, 0)


def _columns(rng):
    """four columns: 17 slices (a 16-byte window plus the next byte) and the three bytes behind them, which no pair may show"""
    return [(rng.integers(0, 256, 17, dtype=np.uint8), rng.integers(0, 256, 3, dtype=np.uint8)) for _ in range(4)]


def _expected_pair(columns, sub):
    b = lambda i, s: int(columns[i][0][s])
    return (b(0, sub) | b(1, sub) << 8 | b(2, sub) << 16 | b(3, sub) << 24, b(0, sub + 1) | b(1, sub + 1) << 8 | b(2, sub + 1) << 16 | b(3, sub + 1) << 24)


def test_selector_sets_equal_the_per_sample_formula():
    """every (base, sub) with sub - base in {0, 1, 2} and sub in 0 .. 15: the pair of the three selector sets is the pair of the per-sample
    alignbyte + perm formula, and both are the slices sub and sub + 1 of the four columns"""
    rng = np.random.default_rng(20261020)
    checked = 0
    for _ in range(8):
        columns = _columns(rng)
        for base in range(16):
            held = [owner_dword(w, n, base) for w, n in columns]
            for sub in range(base, min(base + 2, 15) + 1):
                want = pair_per_sample(columns, sub)
                assert want == _expected_pair(columns, sub), (base, sub)
                assert pair_from_group(held, base, sub) == want, (base, sub)
                checked += 1
    assert checked == 8 * (14 * 3 + 2 + 1)


@pytest.mark.parametrize("forward", (True, False), ids=("up", "down"))
def test_selector_march_over_a_window_in_both_directions(forward):
    """a window marched as the kernel does: cells repeating (several samples per cell) and advancing by one, from every first cell; a sample
    outside its group exchanges again at group_base.  Every pair equals the per-sample formula; a march over all 16 cells needs 6 exchanges"""
    rng = np.random.default_rng(7)
    columns = _columns(rng)
    for start in range(16):
        for repeat in (1, 2, 3):
            cells = range(start, 16) if forward else range(start, -1, -1)
            base, held, exchanges = 64, None, 0
            for sub in (c for c in cells for _ in range(repeat)):
                if not 0 <= sub - base <= 2:
                    base = group_base(forward, sub)
                    held = [owner_dword(w, n, base) for w, n in columns]
                    exchanges += 1
                assert pair_from_group(held, base, sub) == pair_per_sample(columns, sub), (start, repeat, sub, base)
            assert exchanges == -(-len(cells) // 3), (start, repeat, exchanges)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------

_scenes = {}


def _dense_voxels(shape_zyx, seed):
    """every voxel >= 64, noisy: a neighbouring slice or column instead of the right one changes the sample"""
    return np.random.default_rng(seed).integers(64, 256, shape_zyx).astype(np.uint8)


def _thin_open_tf(oracle, shape):
    """no transparent entry (nothing may be skipped: every sample is composited), opacity thin enough that rays stay open to the far face"""
    base = oracle.default_base_tf()
    base[:, 3] = np.float32(min(1.0, 2.0 / max(shape))) * (np.float32(0.15) + np.arange(128, dtype=np.float32) / np.float32(128.0))
    return base


def _dense_scene(oracle, dims_xyz):
    key = ("dense", tuple(dims_xyz))
    if key not in _scenes:
        shape = tuple(dims_xyz)[::-1]
        _scenes[key] = ColumnScene.synthetic(oracle, "dense", _dense_voxels(shape, 20261020 + sum(shape)), _thin_open_tf(oracle, shape), "open, thin")
    return _scenes[key]


def _dims_along(axis, march, lateral):
    """x, y, z extents with `march` cells along `axis` and `lateral` on the two other axes in increasing order"""
    dims = list(lateral)
    dims.insert(axis, march)
    return dims


LIT = (("TRILINEAR lit", 1, 0.6), ("Q8 lit", 2, 0.6))
MARCH_EXTENTS = (3, 4, 5, 15, 16, 17, 18, 31, 33, 49)
STEP_SCALES = (0.37, 0.5, 1.0)


@gpu_test
@pytest.mark.parametrize("extent", MARCH_EXTENTS)
def test_exchange_window_and_group_edges(vr, gpu, oracle, extent):
    """March extents shorter than a group, ragged against it and against the 16-cell window, lateral extents 5 x 7, every voxel dense under an
    open transfer function: every sample is composited, and groups end at the edge between windows w and w + 1.  Step scales 0.37 and 0.5
    (several samples per cell) and 1.0, both signs of all three axes, TRILINEAR lit through the three kernels."""
    gpu.set_window_buffer(BUFFER, BUFFER)
    with edges._policy_restored(gpu):
        for axis in (0, 1, 2):
            scene = _dense_scene(oracle, _dims_along(axis, extent, (5, 7)))
            scene.load(gpu)
            for sign in (1.0, -1.0):
                view = axis_view(vr, scene.dims, axis, sign)
                for scale in STEP_SCALES:
                    p = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, 0.6, 1.0, scale)
                    what = edges._what(scene, p, "TRILINEAR lit", f" step scale {scale:g}")
                    edges._check_frame(vr, gpu, oracle, scene, p, what)
                    assert edges._oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


@gpu_test
@pytest.mark.parametrize("angles", edges.AXIS_POSES, ids=("-z", "-x", "-y", "+x", "+y", "+z"))
def test_exchange_axis_poses_in_both_directions(vr, gpu, oracle, angles):
    """The six axis-aligned orthogonal poses (four of them carry rounding noise in the direction: the kernels with the owner switch) at 32 x 32
    pixels on a dense 16 x 16 x 33 volume with the 33 cells along the march; TRILINEAR and Q8, lit, step scales 0.5 and 1.0."""
    view = vr.custom_view(32, 32, False, angles, 2.0)
    axis = int(np.argmax([abs(view.direction[j]) for j in range(3)]))
    scene = _dense_scene(oracle, _dims_along(axis, 33, (16, 16)))
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with edges._policy_restored(gpu):
        for mode, sampling, kd in LIT:
            for scale in (0.5, 1.0):
                p = column_params(vr, scene, view, sampling, kd, 1.0, scale)
                assert voxel_windows_fit(p, scene.dims, axis)
                edges._check_frame(vr, gpu, oracle, scene, p, edges._what(scene, p, mode, f" pose {angles} step scale {scale:g}"))


# -- flips inside a group

FLIP_POSE, FLIP_DIMS, FLIP_FRAME, FLIP_SCALE = (180.0, 90.0, 0.0), (33, 17, 17), (34, 34), 0.37


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 is exact in fp64)"""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(F)


def flips_between_samples_of_one_cell(view, dims_xyz, step):
    """[(pixel x, pixel y)] of the lanes whose lateral cell changes between two consecutive samples that lie in the SAME cell along the march —
    the second sample reads its pair from the dwords the first one exchanged unless the owner switch ends the group.  Replays pixel_ray and
    the texel-space coordinates of voxcol_march (coordinate = fma(k, dir * half, fma(origin, half, half - 0.5)), lateral cell = (int) of the
    clamped coordinate, cell along the march by truncation) in fp32; waves whose lanes do not share kx (they march per lane) are left out."""
    w, h = int(view.width), int(view.height)
    axis = int(np.argmax([abs(view.direction[j]) for j in range(3)]))
    kx, ky, alive = pixel_segments(view)
    per_lane = {(wx, wy) for wx, wy, _ in mixed_entry_waves(view)}
    fx = (np.arange(w, dtype=np.int64) - w // 2).astype(F)[None, :]
    fy = (np.arange(h, dtype=np.int64) - h // 2).astype(F)[:, None]
    coord = []
    for c in range(3):
        half = F(0.5) * F(dims_xyz[c])
        origin = np.broadcast_to((F(view.origin[c]) + F(view.right_plane[c]) * fx) + F(view.up_plane[c]) * fy, (h, w)).astype(F)
        A, B = F(F(view.direction[c]) * half), _fma(origin, half, half - F(0.5))
        coord.append((A, B, F(dims_xyz[c] - 1)))
    found = []
    for y in range(h):
        for x in range(w):
            if not alive[y, x] or (x // 8, y // 8) in per_lane:
                continue
            ks = [kx[y, x]]
            while ks[-1] + F(step) <= ky[y, x] and len(ks) < 4096:
                ks.append(F(ks[-1] + F(step)))
            ks = np.array(ks, F)
            Am, Bm, _ = coord[axis]
            cell_m = _fma(ks, Am, Bm[y, x]).astype(np.int32)
            for c in range(3):
                if c == axis:
                    continue
                A, B, top = coord[c]
                cell = np.clip(_fma(ks, A, B[y, x]), F(0), top).astype(np.int32)
                change = np.nonzero(cell[1:] != cell[:-1])[0]
                if any(cell_m[n] == cell_m[n + 1] for n in change):
                    found.append((x, y))
    return found


def test_flip_pose_holds_lanes_that_flip_inside_a_group(vr, oracle):
    """the frame of the GPU test below is not vacuous (CPU replay; the view comes from the host library, no GPU needed)"""
    view = vr.custom_view(*FLIP_FRAME, False, FLIP_POSE, 2.0)
    step = F(oracle.default_ray_step(FLIP_DIMS)) * F(FLIP_SCALE)             # column_params' step for this volume
    lanes = flips_between_samples_of_one_cell(view, FLIP_DIMS, step)
    print(f"{len(lanes)} lanes flip between two samples of one cell: {lanes[:8]}")
    assert lanes


@gpu_test
def test_exchange_flips_inside_a_group(vr, gpu, oracle):
    """Pose (180,90,0) — the march along -x, rounding noise in the lateral direction components — on a dense 33 x 17 x 17 volume at 34 x 34
    pixels (0.5 cells per pixel: pixel centres on cell boundaries of the odd lateral extents) and 0.37 of the scene's step: lanes change
    their column between two samples of one cell, inside a group (asserted by the replay with the frame's own step)."""
    scene = _dense_scene(oracle, FLIP_DIMS)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    view = vr.custom_view(*FLIP_FRAME, False, FLIP_POSE, 2.0)
    with edges._policy_restored(gpu):
        for mode, sampling, kd in LIT:
            for scale in (FLIP_SCALE, 0.5):
                p = column_params(vr, scene, view, sampling, kd, 1.0, scale)
                what = edges._what(scene, p, mode, f" pose {FLIP_POSE} step scale {scale:g}")
                assert flips_between_samples_of_one_cell(view, scene.dims, p.ray_step), f"{what}: no lane flips between two samples of one cell"
                edges._check_frame(vr, gpu, oracle, scene, p, what)


# -- holed transfer function

def _banded_voxels(dims_xyz, axis, phase):
    """bands of 2 cells along `axis`, alternately dense (200 .. 255) and transparent (0 .. 15), noisy"""
    shape = tuple(dims_xyz)[::-1]
    rng = np.random.default_rng(99 + axis + 3 * phase)
    dense, clear = rng.integers(200, 256, shape), rng.integers(0, 16, shape)
    index = np.arange(dims_xyz[axis]).reshape([-1 if j == 2 - axis else 1 for j in range(3)])
    return np.where(((index + phase) // 2) % 2 == 0, dense, clear).astype(np.uint8)


def _band_tf(oracle, shape):
    """transparent below entry 64, thin above: the clear bands are skipped sample by sample inside windows that are dense"""
    base = oracle.default_base_tf()
    base[:64, 3] = 0.0
    base[64:, 3] = np.float32(min(1.0, 4.0 / max(shape)))
    return base


@gpu_test
@pytest.mark.parametrize("axis", (0, 1, 2), ids=list(edges.AXES))
def test_exchange_dense_and_transparent_bands(vr, gpu, oracle, axis):
    """Dense and transparent bands alternating every 2 cells along the march (both phases): the composited samples, and with them the
    groups, begin and end at arbitrary cells of a window.  33 cells along the march, 5 x 7 laterally, TRILINEAR and Q8, both signs, step
    scales 0.37 and 1.0."""
    gpu.set_window_buffer(BUFFER, BUFFER)
    dims = _dims_along(axis, 33, (5, 7))
    with edges._policy_restored(gpu):
        for phase in (0, 1):
            key = ("bands", axis, phase)
            if key not in _scenes:
                vox = _banded_voxels(dims, axis, phase)
                _scenes[key] = ColumnScene.synthetic(oracle, f"bands phase {phase}", vox, _band_tf(oracle, vox.shape), "bands")
            scene = _scenes[key]
            scene.load(gpu)
            for sign in (1.0, -1.0):
                view = axis_view(vr, scene.dims, axis, sign)
                for mode, sampling, kd in LIT:
                    for scale in (0.37, 1.0):
                        p = column_params(vr, scene, view, sampling, kd, 1.0, scale)
                        what = edges._what(scene, p, mode, f" step scale {scale:g}")
                        edges._check_frame(vr, gpu, oracle, scene, p, what)
                        assert edges._oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


# ---- the same under the bounds-checked build -------------------------------------------------------------------------------------------

@gpu_test
def test_exchange_under_the_bounds_checked_build():
    """The frames of this file once with build_variants/libvr_hip_bounds.so in a child process (VR_HIP_LIB): every frame still equals the
    oracle and none reports a violation (a violation fails its frame: VrError).  The library is built here when it is missing."""
    if not os.path.exists(BOUNDS_LIB):
        subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), "bounds", "-DVR_BOUNDS_CHECK"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, VR_HIP_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_exchange and not bounds_checked"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
