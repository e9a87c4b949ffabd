"""The aligned run bricks (vr_device.h kRun7*: runs of 8 elements = 32 bytes that cover SEVEN cells, 2048-byte bricks) beside the nine-element
runs: the two copies byte for byte against a numpy construction of the layout, full-march TRILINEAR frames on them against the CPU oracle
and against the nine-element flavour (np.array_equal), the frames that must keep the nine-element flavour, the same frames under the
bounds-checked build, and — without a GPU — the two alignment properties the layout exists for, on the line model's own address function
(scripts/run_lines_model.py)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ColumnScene, column_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "build_variants", "libvr_hip_bounds.so")          # tests/test_gpu_bounds.py's mechanism: VR_HIP_LIB in a child
RUN_LAYOUTS = (2, 3, 6)
KIND_Z, KIND_Y = 13, 14                                                           # bit indices of VR_COPY_RUN7_Z / VR_COPY_RUN7_Y


# ---- CPU: the model's address function ------------------------------------------------------------------------------------------------

def _model():
    spec = importlib.util.spec_from_file_location("run_lines_model", os.path.join(ROOT, "scripts", "run_lines_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _all_cells(nx, no, nr):
    r, o, x = np.meshgrid(np.arange(nr), np.arange(no), np.arange(nx), indexing="ij")
    return x.reshape(-1), o.reshape(-1), r.reshape(-1)


@pytest.mark.parametrize("dims", [(24, 24, 24), (23, 17, 15), (23, 15, 17)])      # (x, other axis, run axis): cubes, and both run directions of 23x17x15
def test_aligned_layout_keeps_pairs_in_32_bytes_and_column_blocks_in_one_line(dims):
    m = _model()
    nx, no, nr = dims
    nbx, nbo = (nx + 7) // 8, (no + 7) // 8
    x, o, r = _all_cells(nx, no, nr)
    off = m.run_offset(7, nbx, nbo, x, o, r)
    # every slice pair (8 bytes) of a 7-cell run lies inside ONE aligned 32-byte block, which is the cell column's run ...
    assert np.array_equal(off // 32, (off + 7) // 32)
    assert np.array_equal(off // 32, m.run_offset(7, nbx, nbo, x, o, (r // 7) * 7) // 32)
    # ... every 2x2 Morton block of cell columns, over the seven cells of a brick, lies in ONE 128-byte line, and no other block shares it
    block = ((r // 7) * (nbo * 4) + (o >> 1)) * (nbx * 4) + (x >> 1)
    line = off // 128
    assert np.array_equal(line, (off + 7) // 128)
    pairs = np.unique(np.stack((block, line), axis=1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
    # distinct cells, distinct addresses; the copy ends where vr_device.h run7_copy_bytes says (without the tail slack)
    assert len(np.unique(off)) == len(off) and off.max() + 8 <= nbx * nbo * ((nr + 6) // 7) * 2048


def test_nine_element_layout_straddles_as_the_design_says():
    """The other layout of the same function: 36-byte runs in 2304-byte bricks.  A run at byte 36 i of its (line-aligned) brick straddles two
    128-byte lines when 36 i mod 128 > 92; 36 i mod 128 = 4 (9 i mod 32) takes each multiple of 4 twice over a brick's 64 runs, eight of the 32
    above 92: 16 runs of 64 (a quarter; of the brick's 17 inner line boundaries the one at byte 1152 = 36 x 32 falls between two runs).  A quarter
    of the slice pairs straddle a 16-byte chunk.  Distinct cells have distinct addresses inside run_copy_bytes."""
    m = _model()
    x, o, r = _all_cells(24, 16, 24)
    off = m.run_offset(9, 3, 2, x, o, r)
    runs = np.unique(m.run_offset(9, 3, 2, x, o, (r >> 3) << 3))
    assert np.count_nonzero(runs // 128 != (runs + 35) // 128) * 64 == 16 * len(runs)
    assert np.count_nonzero(off // 16 != (off + 7) // 16) * 4 == len(off)
    assert len(np.unique(off)) == len(off) and off.max() + 8 <= 3 * 2 * 3 * 2304
    # the aligned layout on the same cells: 1 pair in 7 straddles a chunk (cells 3 of 0..6: bytes 12..19 of the run)
    off7 = m.run_offset(7, 3, 2, x, o, r)
    assert np.array_equal(off7 // 16 != (off7 + 7) // 16, r % 7 == 3)


# ---- GPU: the copies --------------------------------------------------------------------------------------------------------------------

def run7_copy(vox, along_y):
    """[brick: x fastest, then the other axis, then the run axis in steps of SEVEN cells][cell column, 2-D Morton over x and the other axis]
    [k = 0..7 along the run axis, index clamped at the upper face] -> quad element, 4 bytes: the 2x2 neighbourhood across the run axis"""
    z, y, x = vox.shape
    dim_o, dim_r = (z, y) if along_y else (y, z)
    nbx, nbo, nbr = (x + 7) // 8, (dim_o + 7) // 8, (dim_r + 6) // 7
    cell = np.arange(64)
    lx = (cell & 1) | ((cell >> 1) & 2) | ((cell >> 2) & 4)
    lo = ((cell >> 1) & 1) | ((cell >> 2) & 2) | ((cell >> 3) & 4)
    k = np.arange(8)
    pad = lambda n: np.minimum(np.arange(n + 10), n - 1)
    p = vox[np.ix_(pad(z), pad(y), pad(x))]
    out = np.zeros((nbr, nbo, nbx, 64, 8, 4), np.uint8)
    br, bo, bx = np.meshgrid(np.arange(nbr), np.arange(nbo), np.arange(nbx), indexing="ij")
    X = (bx[..., None, None] * 8 + lx[:, None]) + 0 * k
    O = (bo[..., None, None] * 8 + lo[:, None]) + 0 * k
    R = np.minimum(br[..., None, None] * 7 + k + 0 * lx[:, None], dim_r - 1)
    inside = (X < x) & (O < dim_o)
    Xc, Oc = np.minimum(X, x + 8), np.minimum(O, dim_o + 8)
    for i, (dx, do) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        v = p[Oc + do, R, Xc + dx] if along_y else p[R, Oc + do, Xc + dx]
        out[..., i] = np.where(inside, v, 0)
    return out.reshape(-1)


RUN_EXTENTS = (1, 6, 7, 8, 13, 14, 15)          # brick boundaries at multiples of 7, ragged last brick
LATERAL = (1, 5, 8, 9, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("run_extent", RUN_EXTENTS)
def test_aligned_copies_equal_the_host_construction(vr, gpu, run_extent):
    i = RUN_EXTENTS.index(run_extent)
    lat_x, lat_o = LATERAL[i % 5], LATERAL[(i + 2) % 5]
    rng = np.random.default_rng(70 + run_extent)
    # runs along z with this extent, then runs along y with it; the other copy of each volume comes for free (its run axis has a lateral extent)
    for shape in ((run_extent, lat_o, lat_x), (lat_o, run_extent, lat_x)):                      # (z, y, x)
        vox = rng.integers(0, 256, size=shape, dtype=np.uint8)
        gpu.set_layout(vr.LAYOUT_BRICKED)
        gpu.set_volume(vox)
        assert gpu.run_aligned_info()["copies"] == 0
        gpu.prepare(vr.COPY_RUN7_Z | vr.COPY_RUN7_Y)
        info, aligned = gpu.volume_info(), gpu.run_aligned_info()
        want_z, want_y = run7_copy(vox, False), run7_copy(vox, True)
        assert info.copies == vr.COPY_RUN7_Z | vr.COPY_RUN7_Y and info.bricked_bytes == aligned["bytes"] and info.copies_in_policy == vr.COPY_ALL & ~vr.COPY_OCT, shape
        assert aligned["copies"] == vr.COPY_RUN7_Z | vr.COPY_RUN7_Y and aligned["bytes"] == want_z.size + want_y.size + 32 and min(aligned["build_ms"]) > 0, (shape, aligned)
        assert np.array_equal(gpu.download_copy(KIND_Z), want_z), ("aligned runs along z", shape)
        assert np.array_equal(gpu.download_copy(KIND_Y), want_y), ("aligned runs along y", shape)


# ---- GPU: frames ------------------------------------------------------------------------------------------------------------------------

def _holed_random_volume(shape_zyx, seed):
    """random voxels over the whole range, with boxes of zeros punched through (transparent under the default transfer function) and a dense core"""
    rng = np.random.default_rng(seed)
    vox = rng.integers(0, 256, size=shape_zyx, dtype=np.uint8)
    z, y, x = shape_zyx
    vox[z // 3: z // 3 + 4, :, x // 4: x // 4 + 5] = 0
    vox[:, y // 2: y // 2 + 3, :] = 0
    vox[z // 2:, : y // 3, x // 2:] = 0
    return vox


_scenes, _oracle_frames = {}, {}


def _scene(oracle, shape_zyx):
    if shape_zyx not in _scenes:
        _scenes[shape_zyx] = ColumnScene.synthetic(oracle, "holed_random_%dx%dx%d" % shape_zyx[::-1], _holed_random_volume(shape_zyx, 5), None, "default")
    return _scenes[shape_zyx]


def _oracle_frame(oracle, scene, p):
    key = (scene.key, bytes(p))
    if key not in _oracle_frames:
        img = oracle.render(p, scene.vox, scene.tf, scene.esl)
        img.setflags(write=False)
        _oracle_frames[key] = img
    return _oracle_frames[key]


AXIS_POSES = ((0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (180.0, 90.0, 0.0))
# (name, perspective, angles, distance, layouts the frame must run on — None: whatever the policy gives a camera inside the cube)
POSES = (("oblique orthogonal", 0, (-45.0, -45.0, 0.0), 2.0, (6,)),
         ("perspective along axis 0", 1, AXIS_POSES[0], 2.0, (2, 3)), ("perspective along axis 1", 1, AXIS_POSES[1], 2.0, (2, 3)),
         ("perspective along axis 2", 1, AXIS_POSES[2], 2.0, (2, 3)),
         ("oblique perspective", 1, (-45.0, -45.0, 0.0), 2.0, (2, 3)), ("camera inside the cube", 1, (-45.0, -45.0, 0.0), 0.4, None))
SHAPES = ((24, 24, 24), (15, 17, 23))            # (z, y, x): 24^3 and 23 x 17 x 15
FRAMES = ((64, 64), (96, 40))


def _render(gpu, p, flavour):
    gpu.set_run_flavour(flavour)
    try:
        img = gpu.render_volume(p)
        return img, gpu.last_launch()
    finally:
        gpu.set_run_flavour(0)


def _load(vr, gpu, scene):
    gpu.set_layout(vr.LAYOUT_BRICKED)
    scene.load(gpu)
    gpu.set_window_buffer(96, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["24x24x24", "23x17x15"])
def test_full_march_frames_on_aligned_runs_equal_the_oracle_and_the_nine_element_runs(vr, gpu, oracle, shape):
    scene = _scene(oracle, shape)
    _load(vr, gpu, scene)
    for name, perspective, angles, distance, layouts in POSES:
        for w, h in FRAMES:
            view = vr.custom_view(w, h, perspective, angles, distance)
            for kd in (0.6, 0.0):
                p = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, kd, 1.0)
                what = f"{scene.name} {name} {w}x{h} light_kd {kd}"
                want = _oracle_frame(oracle, scene, p)
                seven, info7 = _render(gpu, p, 2)
                nine, info9 = _render(gpu, p, 1)
                assert info7["layout"] == info9["layout"] and (layouts is None or info7["layout"] in layouts), (what, info7, info9)
                on_runs = info7["layout"] in RUN_LAYOUTS
                assert info7["run_flavour"] == (2 if on_runs else 0) and info9["run_flavour"] == (1 if on_runs else 0), (what, info7, info9)
                assert {k: v for k, v in info7.items() if k != "run_flavour"} == {k: v for k, v in info9.items() if k != "run_flavour"}, what
                assert np.array_equal(seven, want), f"{what}: aligned runs differ from the oracle in {int((seven != want).any(-1).sum())} px"
                assert np.array_equal(nine, want), f"{what}: nine-element runs differ from the oracle"
                assert np.array_equal(seven, nine), what
    # the oblique orthogonal frames ran on BOTH copies of either flavour (layout 6) ...
    assert gpu.run_aligned_info()["copies"] == vr.COPY_RUN7_Z | vr.COPY_RUN7_Y
    assert gpu.volume_info().copies & (vr.COPY_RUN_Z | vr.COPY_RUN_Y) == vr.COPY_RUN_Z | vr.COPY_RUN_Y
    # ... and with the copies alternating tile by tile (a frame this small has one block of tiles, hence one copy, under the product's rule) every
    # tile boundary of the frame joins a tile read from the copy along z to one read from the copy along y
    view = vr.custom_view(96, 40, 0, (-45.0, -45.0, 0.0), 2.0)
    p = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, 0.6, 1.0)
    gpu.set_brick_plane(7)
    try:
        for flavour in (2, 1):
            img, info = _render(gpu, p, flavour)
            assert info["layout"] == 6 and info["run_flavour"] == flavour and info["tiles_x"] * info["tiles_y"] >= 2, info
            assert np.array_equal(img, _oracle_frame(oracle, scene, p)), ("alternating tiles", flavour)
    finally:
        gpu.set_brick_plane(-1)


@pytest.mark.gpu
def test_automatic_flavour_and_the_frames_that_keep_nine_element_runs(vr, gpu, oracle):
    """Automatic policy: a full-march frame on run bricks reads what vr_hip_set_run_flavour(0) stands for — either flavour, the oracle's image;
    a frame with early termination (threshold 0.95) and one with leaping report the nine-element flavour under every setting and build no aligned copy."""
    scene = _scene(oracle, SHAPES[1])
    _load(vr, gpu, scene)
    view = vr.custom_view(64, 64, 1, (-45.0, -45.0, 0.0), 2.0)
    for flavour in (0, 2, 1):
        ert = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, 0.6, 0.95)
        leap = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, 0.6, 1.0)
        leap.esl = 1
        for what, p in (("early termination", ert), ("leaping", leap)):
            img, info = _render(gpu, p, flavour)
            assert info["layout"] in (2, 3) and info["run_flavour"] == 1, (what, flavour, info)
            assert np.array_equal(img, _oracle_frame(oracle, scene, p)), (what, flavour)
    assert gpu.run_aligned_info()["copies"] == 0 and gpu.volume_info().copies & (vr.COPY_RUN7_Z | vr.COPY_RUN7_Y) == 0
    full = column_params(vr, scene, view, vr.SAMPLE_TRILINEAR, 0.6, 1.0)
    img, info = _render(gpu, full, 0)
    assert info["layout"] in (2, 3) and info["run_flavour"] in (1, 2), info
    assert (info["run_flavour"] == 2) == (gpu.run_aligned_info()["copies"] != 0)
    assert np.array_equal(img, _oracle_frame(oracle, scene, full))
    with pytest.raises(vr.VrError) as e:
        gpu.set_run_flavour(3)
    assert e.value.code == 1


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(BOUNDS_LIB), reason="build_variants/libvr_hip_bounds.so not built (scripts/build_variant.sh bounds -DVR_BOUNDS_CHECK)")
def test_frames_under_the_bounds_checked_build():
    """The frame tests of this file once with the -DVR_BOUNDS_CHECK library in a child process: every gather of the march held against the aligned
    copies' own extents (bc_bytes / bc_alt_bytes), every table index against its padded table — a violation fails its frame (VrError)."""
    env = dict(os.environ, VR_HIP_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "full_march_frames or automatic_flavour"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
