"""voxcol_pairs_kernel: the TRILINEAR column march over the voxel windows whose explicit fetches (the shading sample, the per-lane march)
read one element pair from the quad-element windows instead of eight bytes from the voxel windows.  Build checks on the CPU tier — the
limits tests/test_voxcol_march.py holds voxcol_tri_kernel to —; on the GPU its frames equal the byte-load kernel's (mode 2),
colmarch_kernel's (mode 1) and the oracle's byte for byte, unlit frames never build the second copy, and a context that cannot build it
renders the same image through the byte loads."""
import os
import re

import numpy as np
import pytest

from test_abi import _disassemble_gfx950, _no_spill_kernels, _walk_gathers_in_flight
from test_voxcol_march import _ortho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = r"voxcol_pairs_kernelILi(\d)ELi(\d)ELb([01])E"
POSES = ((0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (180.0, 90.0, 0.0), (0.0, 90.0, 0.0), (270.0, 0.0, 0.0), (0.0, 180.0, 0.0), (90.0, 90.0, 0.0), (0.0, 0.0, 90.0))
FRAMES = (("bucky", "bench64_view1_default", 256, 256), ("bucky", "bench64_view1_default", 130, 67), ("blob_40x24x56", "view1_default", 192, 160))


def test_voxcol_pairs_kernels_keep_eight_waves_without_spills(vr):
    """{TRILINEAR, Q8} x {x, y, z} x {with, without flips} = 12 instantiations: <= 80 SGPRs, <= 64 VGPRs, no scratch, no spills."""
    import subprocess
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    log = os.path.join(csrc, "resource_usage.log")
    if not os.path.exists(log):
        subprocess.check_call(["make", "-B", "-C", csrc])
    found = _no_spill_kernels(open(log).read(), KERNEL)
    assert len(found) == 12, sorted(found)


def test_voxcol_pairs_gathers_in_flight_are_untouched(vr, tmp_path):
    """The walk of tests/test_abi.py over the disassembly with the minimum counts of the voxcol_tri_kernel test: the plain 8-byte load of
    the shading sample must not make any instruction name a register of a window gather that is still in flight."""
    funcs = _disassemble_gfx950(vr.library_path(), tmp_path)
    checked = 0
    for name, lines in funcs.items():
        if re.search(KERNEL, name) is None:
            continue
        checked += 1
        _walk_gathers_in_flight(name, lines, set(), 8, 4)
    assert checked == 12, checked


_oracle_frames = {}


def _case(golden, name, label):
    return [c for c in golden.cases(True) if c["label"] == label and c["volume"] == name][0]


def _oracle_frame(oracle, golden, vr, name, label, w, h, angles, samp, kd, step_scale):
    """The oracle's frame of one parameter set, computed once for all tests of this file."""
    key = (name, w, h, angles, samp, kd, step_scale)
    if key not in _oracle_frames:
        st = golden.volume_state(name)
        p = _ortho(vr, golden, _case(golden, name, label), name, samp, w, h, angles, 2.0, kd, step_scale)
        _oracle_frames[key] = oracle.render(p, golden.voxels(name), st["tf"], st["esl"])
    return _oracle_frames[key]


def _load(gpu, golden, name, w, h):
    st = golden.volume_state(name)
    gpu.set_transfer_fn(st["tf"], st["esl"])
    gpu.set_volume(golden.voxels(name))
    gpu.set_window_buffer(w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("name,label,w,h", FRAMES, ids=["bucky-256x256", "bucky-130x67", "blob-192x160"])
def test_voxcol_pairs_equals_byte_loads_colmarch_and_oracle(vr, gpu, golden, oracle, name, label, w, h):
    """Byte for byte, lit TRILINEAR and lit Q8 at step scale 0.37, the eight poses of the voxel-window parity test (flips at (180,90,0),
    reversed directions): mode 0 shades from the pair copy, mode 2 by byte loads, mode 1 is colmarch_kernel.  40x24x56 has march extents
    that are multiples of neither 3 nor 16: both copies end in a ragged window and the clamps at the upper faces are exercised."""
    _load(gpu, golden, name, w, h)
    try:
        for angles in POSES:
            for samp, kd, step_scale in ((vr.SAMPLE_TRILINEAR, 0.6, 1.0), (vr.SAMPLE_TRILINEAR_Q8, 0.6, 0.37)):
                what = (name, w, h, angles, samp, kd, step_scale)
                p = _ortho(vr, golden, _case(golden, name, label), name, samp, w, h, angles, 2.0, kd, step_scale)
                gpu.set_column_copy(0)
                pairs = gpu.render_volume(p)
                info = gpu.last_launch()
                assert info["layout"] == 7 and info["column_voxels"] == 1 and info["column_shade_pairs"] == 1, (what, info)
                assert gpu.volume_info().copies & (vr.COPY_COL_X << info["brick_plane"]), what
                gpu.set_column_copy(2)
                bytewise = gpu.render_volume(p)
                info = gpu.last_launch()
                assert info["layout"] == 7 and info["column_voxels"] == 1 and info["column_shade_pairs"] == 0, (what, info)
                gpu.set_column_copy(1)
                quad = gpu.render_volume(p)
                info = gpu.last_launch()
                assert info["layout"] == 7 and info["column_voxels"] == 0 and info["column_shade_pairs"] == 0, (what, info)
                assert np.array_equal(pairs, bytewise), what
                assert np.array_equal(pairs, quad), what
                assert np.array_equal(pairs, _oracle_frame(oracle, golden, vr, name, label, w, h, angles, samp, kd, step_scale)), what
    finally:
        gpu.set_column_copy(0)


@pytest.mark.gpu
def test_unlit_frames_do_not_build_the_pair_copy(vr, gpu, golden):
    """light_kd = 0: nothing is shaded, so the frame reports column_shade_pairs 0 and builds no quad-element window copy."""
    name, label, w, h = FRAMES[2]
    _load(gpu, golden, name, w, h)
    gpu.set_column_copy(0)
    col_bits = vr.COPY_COL_X | vr.COPY_COL_Y | vr.COPY_COL_Z
    before = gpu.volume_info().copies
    for angles in POSES[:3]:
        p = _ortho(vr, golden, _case(golden, name, label), name, vr.SAMPLE_TRILINEAR, w, h, angles, 2.0, 0.0, 1.0)
        gpu.render_volume(p)
        info = gpu.last_launch()
        assert info["layout"] == 7 and info["column_voxels"] == 1 and info["column_shade_pairs"] == 0, (angles, info)
    assert gpu.volume_info().copies & col_bits == before & col_bits == 0


@pytest.mark.gpu
def test_lit_frame_without_the_pair_copy_shades_by_byte_loads(vr, golden, oracle):
    """vr_hip_release_linear_copy permits a context that holds nothing but the voxel windows; the pair copy can then not be built any more,
    and a lit frame in mode 0 goes through the byte-load kernel with the same image (and builds nothing)."""
    name, label, w, h = FRAMES[2]
    r = vr.HipRenderer(0)
    try:
        _load(r, golden, name, w, h)
        voxel_windows = vr.COPY_COLV_X | vr.COPY_COLV_Y | vr.COPY_COLV_Z
        r.prepare(voxel_windows)
        r.release_linear_copy()
        assert r.volume_info().copies == voxel_windows
        for angles in POSES[:3]:
            p = _ortho(vr, golden, _case(golden, name, label), name, vr.SAMPLE_TRILINEAR, w, h, angles, 2.0, 0.6, 1.0)
            img = r.render_volume(p)
            info = r.last_launch()
            assert info["layout"] == 7 and info["column_voxels"] == 1 and info["column_shade_pairs"] == 0, (angles, info)
            assert np.array_equal(img, _oracle_frame(oracle, golden, vr, name, label, w, h, angles, vr.SAMPLE_TRILINEAR, 0.6, 1.0)), angles
        assert r.volume_info().copies == voxel_windows
    finally:
        r.close()
