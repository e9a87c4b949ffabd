"""The four column marches (colmarch_kernel, colmarch_nearest_kernel, voxcol_tri_kernel, voxcol_pairs_kernel) away from the one corner the
other column tests hold them in: early ray termination, march extents shorter than a window and ragged against it, lateral extents below a
4x4 block, transfer functions that forbid / allow / interleave window skipping, and cameras inside the cube.  Every frame is compared byte
for byte with the CPU oracle, every frame asserts the launch record of the kernel it claims to test, and every frame with a threshold below
1 outside the single-slice volumes asserts that the oracle really terminates rays in it (its sample count against the full march's)."""
import contextlib

import numpy as np
import pytest

from helpers import ColumnScene, axis_view, column_params, compare_frames, smooth_noisy_volume, voxel_windows_fit

pytestmark = pytest.mark.gpu

BUFFER = 128                                    # window buffer edge: every frame of this file fits (the largest is 100 x 86)
RATIO_BAND = (0.25, 0.90)                       # samples with the threshold / samples of the full march: termination bites, but not in the first window
AXES = "xyz"


@contextlib.contextmanager
def _policy_restored(gpu):
    try:
        yield gpu
    finally:
        gpu.set_column_copy(0)
        gpu.set_brick_plane(-1)
        gpu.set_tile_mapping(-1)


# ---- the oracle's frames: each computed once, shared by every test of this file, never written to ---------------------------------------

_oracle_frames = {}


def _oracle_frame(oracle, scene, p):
    """(frame, samples taken) of the CPU oracle for one parameter set."""
    key = (scene.key, bytes(p))
    if key not in _oracle_frames:
        img, st = oracle.render(p, scene.vox, scene.tf, scene.esl, stats=True)
        img.setflags(write=False)
        _oracle_frames[key] = (img, int(st.samples))
    return _oracle_frames[key]


def _sample_ratio(oracle, scene, p):
    full = p.copy()
    full.ray_threshold = 1.0
    return _oracle_frame(oracle, scene, p)[1] / max(1, _oracle_frame(oracle, scene, full)[1])


def _assert_termination_bites(oracle, scene, p, what):
    ratio = _sample_ratio(oracle, scene, p)
    assert RATIO_BAND[0] <= ratio <= RATIO_BAND[1], f"{what}: the oracle takes {ratio:.3f} of the full march's samples, outside {RATIO_BAND}"


# ---- one frame through the kernels of its mode -------------------------------------------------------------------------------------

def _what(scene, p, mode, extra=""):
    d = [p.view.direction[j] for j in range(3)]
    axis = int(np.argmax(np.abs(d)))
    return (f"volume {scene.name} {scene.vox.shape} tf {scene.tf_name} axis {AXES[axis]} sign {'+' if d[axis] > 0 else '-'} mode {mode} "
            f"threshold {p.ray_threshold:g} frame {p.view.width}x{p.view.height}{extra}")


def _check_frame(vr, gpu, oracle, scene, p, what, voxel_windows=True, copies=(0, 1, 2)):
    """TRILINEAR / Q8: vr_hip_set_column_copy 0 (voxel windows, lit frames shade from the element pairs: voxcol_pairs_kernel), 2 (voxel
    windows, byte loads: voxcol_tri_kernel) and 1 (quad-element windows: colmarch_kernel); NEAREST: colmarch_nearest_kernel.  Each must
    report itself in the launch record and give the oracle's bytes.  voxel_windows = False: the host declines the voxel windows for this
    frame (the caller says why) and all three modes run colmarch_kernel."""
    want = _oracle_frame(oracle, scene, p)[0]
    nearest = p.sampling == vr.SAMPLE_NEAREST
    for copy in (0,) if nearest else copies:
        gpu.set_column_copy(copy)
        img = gpu.render_volume(p)
        info = gpu.last_launch()
        voxcol = int(not nearest and copy != 1 and voxel_windows)
        pairs = int(voxcol and copy == 0 and p.light_kd > 0.01)
        assert info["layout"] == 7 and info["column_voxels"] == voxcol and info["column_shade_pairs"] == pairs, f"{what} column copy {copy}: launched {info}"
        ndiff, maxd = compare_frames(img, want)
        assert ndiff == 0, f"{what} column copy {copy}: {ndiff} px differ from the oracle, max delta {maxd}"
    gpu.set_column_copy(0)


FOUR_KERNELS = (("TRILINEAR lit", 1, 0.6, 1.0), ("NEAREST lit", 0, 0.6, 1.0))          # (mode, sampling, light_kd, step scale): 3 + 1 kernels


def _axis_cases(vr, scene, modes, thresholds, cells_per_pixel=0.5, distances=(2.0,), shift=0.3, margin=8, axes=(0, 1, 2)):
    """(params, what) for both signs of every axis, every mode and threshold, over hand-built views."""
    for axis in axes:
        for sign in (1.0, -1.0):
            for distance in distances:
                view = axis_view(vr, scene.dims, axis, sign, cells_per_pixel, distance, shift, margin)
                for mode, sampling, kd, step_scale in modes:
                    for threshold in thresholds:
                        p = column_params(vr, scene, view, sampling, kd, threshold, step_scale)
                        yield p, _what(scene, p, mode, f" distance {distance:g}")


# ---- A. early termination ----------------------------------------------------------------------------------------------------------

A_FRAMES = (("bucky", 96, 96), ("bucky", 75, 50), ("blob_40x24x56", 96, 96))
A_IDS = ["bucky-96x96", "bucky-75x50", "blob-96x96"]
# -z, -x, -y, +x, +y, +z; all but the first and the fifth carry rounding noise of 1e-8 .. 9e-8 in the direction (flips, careful windows)
AXIS_POSES = ((0.0, 0.0, 0.0), (180.0, 90.0, 0.0), (90.0, 0.0, 0.0), (0.0, 90.0, 0.0), (270.0, 0.0, 0.0), (0.0, 180.0, 0.0))
OBLIQUE_POSES = ((0.02, 0.0, 0.0), (90.0, 0.013, 0.0), (-45.0, -45.0, 0.0), (1.5, 2.5, 0.0))      # forced: mostly the per-lane march
THRESHOLDS = (0.5, 0.8, 0.95)
A_MODES = (("TRILINEAR lit", 1, 0.6, None), ("Q8 lit step 0.37", 2, 0.6, 0.37), ("Q8 unlit", 2, 0.0, None), ("NEAREST lit", 0, 0.6, None), ("NEAREST unlit", 0, 0.0, None))
# The step of the modes that leave it open (None above): the volume's default, except where the oracle says that termination then hardly
# bites.  40x24x56 under its own transfer function is thin: at the default step a threshold of 0.95 cuts only 8 - 11 % of the samples from
# +x, -y and +z (ratios 0.89 .. 0.92 on the oracle, outside the band); at 0.7 of the step the same opacity is taken 1.4 times as often and
# the ratios are 0.82 .. 0.87.
A_STEP_SCALE = {("blob_40x24x56", 0.95): 0.7}

_scenes = {}


def _golden_scene(golden, name):
    if name not in _scenes:
        _scenes[name] = ColumnScene.from_golden(golden, name)
    return _scenes[name]


def _pose_params(vr, scene, angles, w, h, sampling, kd, threshold, step_scale):
    return column_params(vr, scene, vr.custom_view(w, h, False, angles, 2.0), sampling, kd, threshold, step_scale)


def _ert_pose_cases(vr, scene, w, h, threshold):
    """(params, what, forced) of section A for one frame size and threshold"""
    for angles in AXIS_POSES + OBLIQUE_POSES:
        for mode, sampling, kd, step_scale in A_MODES:
            if step_scale is None:
                step_scale = A_STEP_SCALE.get((scene.name, threshold), 1.0)
            p = _pose_params(vr, scene, angles, w, h, sampling, kd, threshold, step_scale)
            yield p, _what(scene, p, mode, f" pose {angles} step scale {step_scale:g}"), angles in OBLIQUE_POSES


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name,w,h", A_FRAMES, ids=A_IDS)
def test_column_edges_early_termination(vr, gpu, golden, oracle, name, w, h, threshold):
    """Orthogonal views along -z, -x, -y, +x, +y, +z under the automatic policy, and the near-axis and oblique poses of the column parity
    test forced into the column kernels (their per-lane march), with ray thresholds below 1: the ERT line of col_tri_sample (three kernels)
    and colmarch_nearest_kernel's own, the open-lane term of the window-skip decision, and the shared k batch that keeps marching for the
    lanes still open.  All three TRILINEAR paths agree with each other through the oracle's frame."""
    scene = _golden_scene(golden, name)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for p, what, forced in _ert_pose_cases(vr, scene, w, h, threshold):
            _assert_termination_bites(oracle, scene, p, what)
            gpu.set_brick_plane(8 if forced else -1)
            # forced frames: the voxel windows where the wave's rectangle of columns fits (the host's condition, restated)
            d = [abs(p.view.direction[j] * scene.dims[j]) for j in range(3)]
            _check_frame(vr, gpu, oracle, scene, p, what, voxel_windows=voxel_windows_fit(p, scene.dims, int(np.argmax(d))) if forced else True)


@pytest.mark.parametrize("name,w,h", A_FRAMES, ids=A_IDS)
def test_column_edges_early_termination_bands_and_tile_phases(vr, gpu, golden, oracle, name, w, h):
    """Threshold 0.8 on the pose with flips, (180,90,0): forced tile phases and lane maps move the waves over the cell columns (5 and 10 add
    the wave-shape bits, which the column kernels must ignore), and a partition into 3 ranks of 16-row bands changes which rows a wave holds."""
    scene = _golden_scene(golden, name)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    frames = [(mode, _pose_params(vr, scene, (180.0, 90.0, 0.0), w, h, sampling, 0.6, 0.8, 1.0)) for mode, sampling in (("TRILINEAR lit", 1), ("NEAREST lit", 0))]
    with _policy_restored(gpu):
        for mode, p in frames:
            _assert_termination_bites(oracle, scene, p, _what(scene, p, mode))
            for lane_map in (0, 1, 2, 5, 10):
                for phase in ((0, 0), (3, 5), (7, 1)):
                    gpu.set_tile_mapping(lane_map, *phase)
                    _check_frame(vr, gpu, oracle, scene, p, _what(scene, p, mode, f" lane map {lane_map} phase {phase}"))
            gpu.set_tile_mapping(-1)
            for rank in range(3):
                pb, _ = vr.band_partition(p.copy(), rank, 3, 16)
                _check_frame(vr, gpu, oracle, scene, pb, _what(scene, pb, mode, f" band rank {rank} of 3, 16 rows"))


# ---- B. ragged extents -----------------------------------------------------------------------------------------------------------------

# (z, y, x).  March extents over the three axes: 1, 2, 3, 4, 15, 16, 17, 33, 47, 48, 49 (and 5, 7, 9, 19, 31); lateral extents 1, 2, 3, 5, 9, 17 among them
RAGGED_SHAPES = ((1, 5, 7), (2, 3, 17), (3, 4, 16), (4, 15, 33), (16, 17, 5), (17, 31, 3), (47, 6, 2), (48, 2, 9), (49, 9, 4), (5, 1, 19))


def _shape_id(shape):
    return "x".join(str(n) for n in shape)


def _ragged_voxels(shape):
    return smooth_noisy_volume(shape, 20261018 + sum(shape))


def _thin_base_tf(oracle, shape, per_ray=6.0):
    """The default base transfer function with its opacity scaled by per_ray / (longest edge): a ray through the whole cube takes about as
    many samples as the longest edge has cells (the reference's default step), and an accumulated opacity of 0.8 then needs a good part of
    them.  With the unscaled opacity (up to 0.9 per sample) rays through these fields end inside their first window."""
    base = oracle.default_base_tf()
    base[:, 3] *= np.float32(min(1.0, per_ray / max(shape)))
    return base


def _ragged_scene(oracle, shape):
    key = ("ragged", shape)
    if key not in _scenes:
        _scenes[key] = ColumnScene.synthetic(oracle, "ragged", _ragged_voxels(shape), _thin_base_tf(oracle, shape), "default, opacity x 6/edge")
    return _scenes[key]


@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=_shape_id)
def test_column_edges_ragged_extents(vr, gpu, oracle, shape):
    """Synthetic volumes whose march extents are shorter than a window (3 cells, 16 cells), one cell past one, one short of one, and whose
    lateral extents are below a 4x4 block of columns or one past it: col_first_window, col_window_budget, the last ragged window, the +1
    neighbour at the upper face, nrect against tiny rectangles.  Both signs of every axis, four kernels, thresholds 1.0 and 0.8, frames at
    0.5 cells per pixel with a margin of empty pixels."""
    scene = _ragged_scene(oracle, shape)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for p, what in _axis_cases(vr, scene, FOUR_KERNELS, (1.0, 0.8)):
            if p.ray_threshold < 1.0:
                _assert_termination_bites(oracle, scene, p, what)
            _check_frame(vr, gpu, oracle, scene, p, what)


# ---- C. transfer functions ---------------------------------------------------------------------------------------------------------

def _strength(shape):
    """opacity per sample that lets a ray through the whole cube (about as many samples as the longest edge has cells) reach 0.8 part-way"""
    return np.float32(min(1.0, 6.0 / max(shape)))


def _open_tf(oracle, shape):
    """no leading zero entry: nothing may be skipped (skip_mask 0, skip_cmp 1)"""
    base = oracle.default_base_tf()
    base[:, 3] = _strength(shape) * (np.float32(0.15) + np.arange(128, dtype=np.float32) / np.float32(128.0))
    return base


def _sparse_tf(oracle, shape):
    """entries 0 .. 99 transparent: most windows are skippable"""
    base = oracle.default_base_tf()
    base[:100, 3] = 0.0
    base[100:, 3] = np.float32(0.35)
    return base


def _holed_tf(oracle, shape):
    """runs of 8 entries, alternately transparent and opaque, from a transparent one: the holes lie above the skip threshold"""
    base = oracle.default_base_tf()
    base[:, 3] = np.where((np.arange(128) // 8) % 2 == 1, np.float32(1.5) * _strength(shape), np.float32(0.0))
    return base


TFS = {"open": _open_tf, "sparse": _sparse_tf, "holes": _holed_tf}
C_VOLUMES = ("blob_40x24x56", (16, 17, 5), (49, 9, 4))


def _tf_scene(oracle, golden, volume, tf_name):
    key = ("tf", volume, tf_name)
    if key not in _scenes:
        vox, name = (golden.voxels(volume), volume) if isinstance(volume, str) else (_ragged_voxels(volume), "ragged")
        _scenes[key] = ColumnScene.synthetic(oracle, name, vox, TFS[tf_name](oracle, vox.shape), tf_name)
    return _scenes[key]


@pytest.mark.parametrize("tf_name", sorted(TFS))
@pytest.mark.parametrize("volume", C_VOLUMES, ids=lambda v: v if isinstance(v, str) else _shape_id(v))
def test_column_edges_transfer_functions(vr, gpu, golden, oracle, volume, tf_name):
    """What may be skipped is the transfer function's: with opacity at entry 0 no window is skippable, with 100 leading zeros most are, and
    windows whose voxels fall into opacity holes above the skip threshold must be marched.  Thresholds 1.0 and 0.8, four kernels."""
    scene = _tf_scene(oracle, golden, volume, tf_name)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    blob = isinstance(volume, str)
    with _policy_restored(gpu):
        for p, what in _axis_cases(vr, scene, FOUR_KERNELS, (1.0, 0.8), cells_per_pixel=0.6 if blob else 0.5, margin=6 if blob else 8):
            if p.ray_threshold < 1.0 and tf_name != "sparse":       # (sparse: most rays meet nothing visible and no ray count can fall far)
                _assert_termination_bites(oracle, scene, p, what)
            elif p.ray_threshold < 1.0:
                assert _sample_ratio(oracle, scene, p) < 1.0, what                     # some ray does end early
            _check_frame(vr, gpu, oracle, scene, p, what)
            assert _oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


SLAB_EXTENT = 34
SLABS = (0, 2, 3, 15, 16, 17, SLAB_EXTENT - 1)
SLAB_MODES = (("TRILINEAR lit step 0.2", 1, 0.6, 0.2), ("TRILINEAR lit", 1, 0.6, 1.0), ("NEAREST lit", 0, 0.6, 1.0))


def _slab_scene(oracle, axis, m):
    key = ("slab", axis, m)
    if key not in _scenes:
        dims = [5, 9]
        dims.insert(axis, SLAB_EXTENT)                                           # x, y, z
        vox = np.zeros(dims[::-1], np.uint8)
        index = [slice(None)] * 3
        index[2 - axis] = m
        vox[tuple(index)] = 255
        _scenes[key] = ColumnScene.synthetic(oracle, f"slab {m} along {AXES[axis]}", vox, _sparse_tf(oracle, vox.shape), "sparse")
    return _scenes[key]


@pytest.mark.parametrize("axis", (0, 1, 2), ids=list(AXES))
def test_column_edges_single_slices_under_the_sparse_tf(vr, gpu, oracle, axis):
    """One slice of 255 in a volume of zeroes, 34 cells along the march: a window is dense only through that slice, and a sample in the cell
    below it — the last cell of the window before, where the slice is a window's first (3, 15 and 16 -> 15, 16) — depends on exactly one
    slice of the neighbouring window.  One TRILINEAR step is a fifth of the default, under 0.2 cells: the sparse transfer function shows a
    sample within 0.22 cells of the slice, so at least one sample on each side of it is visible; the default step runs as well.  No
    sample-ratio condition here: a ray meets one opaque slice, and how much of the empty rest is cut depends on where that slice lies."""
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for m in SLABS:
            scene = _slab_scene(oracle, axis, m)
            scene.load(gpu)
            for p, what in _axis_cases(vr, scene, SLAB_MODES, (1.0, 0.8), axes=(axis,)):
                _check_frame(vr, gpu, oracle, scene, p, what)
                if p.sampling == vr.SAMPLE_NEAREST or p.ray_step < 0.5 * float(scene.ray_step):       # (at the default step the samples may all miss the slice)
                    assert _oracle_frame(oracle, scene, p)[0][..., 3].any(), f"{what}: the oracle's frame is empty"


# ---- D. the camera inside the cube -------------------------------------------------------------------------------------------------

D_VOLUMES = ("blob_40x24x56", (16, 17, 5))


def _inside_scene(oracle, golden, volume):
    """Rays from the centre are half as long as rays through the whole cube: the synthetic field gets the default opacity times
    12 / (longest edge), twice section B's.  40x24x56 gets the default base transfer function as it is: half of its voxels lie below that
    function's visible range, and with its own, thinner one a threshold of 0.8 cuts less than a tenth of these short rays' samples."""
    key = ("inside", volume)
    if key not in _scenes:
        if isinstance(volume, str):
            _scenes[key] = ColumnScene.synthetic(oracle, volume, golden.voxels(volume), oracle.default_base_tf(), "default base")
        else:
            _scenes[key] = ColumnScene.synthetic(oracle, "ragged", _ragged_voxels(volume), _thin_base_tf(oracle, volume, 12.0), "default, opacity x 12/edge")
    return _scenes[key]


@pytest.mark.parametrize("volume", D_VOLUMES, ids=lambda v: v if isinstance(v, str) else _shape_id(v))
def test_column_edges_camera_inside_the_cube(vr, gpu, golden, oracle, volume):
    """The origin on the axis 0.4 before the centre and at the centre: kx = 0, the first window is one in the middle of the column and is
    entered part-way through.  Both signs of every axis, TRILINEAR lit (three kernels) and NEAREST, thresholds 1.0 and 0.8."""
    scene = _inside_scene(oracle, golden, volume)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    blob = isinstance(volume, str)
    with _policy_restored(gpu):
        for p, what in _axis_cases(vr, scene, FOUR_KERNELS, (1.0, 0.8), cells_per_pixel=0.6 if blob else 0.5, distances=(0.4, 0.0), margin=6 if blob else 8):
            if p.ray_threshold < 1.0:
                _assert_termination_bites(oracle, scene, p, what)
            _check_frame(vr, gpu, oracle, scene, p, what)


@pytest.mark.parametrize("volume", D_VOLUMES, ids=lambda v: v if isinstance(v, str) else _shape_id(v))
def test_column_edges_camera_inside_pixels_on_cell_boundaries(vr, gpu, golden, oracle, volume):
    """The same origins with a pixel pitch of exactly one cell and no half-pixel shift: pixel centres lie at whole cells from the volume's
    centre — on voxel boundaries of a NEAREST sample for even extents (40x24x56) and on the cell boundaries of a trilinear one for odd ones
    (the lateral extents 17 and 5, 5 of the ragged shape).  POLICY: at one cell per pixel a wave's rectangle of columns is
    (floor(7 * 1.0) + 4)^2 = 121 > 64 lanes, so the host declines the voxel windows for both shapes (vr_hip_api.cpp, `voxcol`), forced
    (vr_hip_set_brick_plane(8)) as well — the force does not reach that condition — and all three TRILINEAR modes run colmarch_kernel: the
    fallback image is asserted under both settings."""
    scene = _inside_scene(oracle, golden, volume)
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for p, what in _axis_cases(vr, scene, FOUR_KERNELS, (1.0, 0.8), cells_per_pixel=1.0, distances=(0.4, 0.0), shift=0.0):
            march = int(np.argmax([abs(p.view.direction[j]) for j in range(3)]))
            assert not voxel_windows_fit(p, scene.dims, march), what
            if p.ray_threshold < 1.0:
                _assert_termination_bites(oracle, scene, p, what)
            for plane in (-1, 8):
                gpu.set_brick_plane(plane)
                _check_frame(vr, gpu, oracle, scene, p, what + f" brick plane {plane}", voxel_windows=False)


# ---- out of scope for these kernels ------------------------------------------------------------------------------------------------

def test_column_edges_two_byte_voxels_never_take_the_column_kernels(vr, gpu, golden, oracle):
    """A u16 volume on an axis pose: another layout, the oracle's image."""
    st = golden.volume_state("bucky")
    scene = ColumnScene("bucky u16", golden.voxels("bucky").astype(np.uint16) * 257, st["tf"], st["esl"], st["esl_block_dims"], st["esl_block_size"], st["ray_step"])
    scene.load(gpu)
    gpu.set_window_buffer(BUFFER, BUFFER)
    with _policy_restored(gpu):
        for sampling in (vr.SAMPLE_TRILINEAR, vr.SAMPLE_NEAREST):
            p = _pose_params(vr, scene, (0.0, 0.0, 0.0), 96, 96, sampling, 0.6, 0.8, 1.0)
            img = gpu.render_volume(p)
            assert gpu.last_launch()["layout"] != 7, gpu.last_launch()
            assert compare_frames(img, _oracle_frame(oracle, scene, p)[0]) == (0, 0), _what(scene, p, sampling)
