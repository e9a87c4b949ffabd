"""voxcol_tri_kernel: the TRILINEAR column march over the windows of 16 plain voxels (kLayoutVoxCol).  Build checks on the CPU tier
(registers, spills, the hand-counted gather pipeline); on the GPU its frames equal colmarch_kernel's and the oracle's byte for byte,
and the host takes it only where a wave's column rectangle fits in 64 lanes."""
import math
import os
import re

import numpy as np
import pytest

from test_abi import _disassemble_gfx950, _no_spill_kernels, _walk_gathers_in_flight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = r"voxcol_tri_kernelILi(\d)ELi(\d)ELb([01])E"


def test_voxcol_kernels_keep_eight_waves_without_spills(vr):
    """{TRILINEAR, Q8} x {x, y, z} x {with, without flips} = 12 instantiations: <= 80 SGPRs, <= 64 VGPRs, no scratch, no spills."""
    import subprocess
    csrc = os.path.join(ROOT, "volume-rendering_amd", "csrc")
    log = os.path.join(csrc, "resource_usage.log")
    if not os.path.exists(log):
        subprocess.check_call(["make", "-B", "-C", csrc])
    found = _no_spill_kernels(open(log).read(), KERNEL)
    assert len(found) == 12, sorted(found)


def test_voxcol_gathers_in_flight_are_untouched(vr, tmp_path):
    """tests/test_abi.py's walk over the disassembly, for this kernel (no sink registers): no instruction names a register of a managed
    gather that the hand-counted s_waitcnt vmcnt(N) has not retired yet."""
    funcs = _disassemble_gfx950(vr.library_path(), tmp_path)
    checked = 0
    for name, lines in funcs.items():
        if re.search(KERNEL, name) is None:
            continue
        checked += 1
        _walk_gathers_in_flight(name, lines, set(), 8, 4)
    assert checked == 12, checked


def _ortho(vr, golden, case, name, samp, w, h, angles, zoom, kd, step_scale):
    p = golden.params(case, samp)
    v = vr.custom_view(w, h, False, angles, zoom)
    for f in ("origin", "direction", "right_plane", "up_plane"):
        for j in range(3):
            getattr(p.view, f)[j] = getattr(v, f)[j]
    p.view.width, p.view.height, p.view.perspective = w, h, 0
    p = vr.whole_frame(p)
    p.esl, p.ray_threshold, p.light_kd = 0, 1.0, kd
    p.ray_step = float(np.float32(p.ray_step) * np.float32(step_scale))
    return p


@pytest.mark.gpu
def test_voxcol_march_equals_colmarch_and_oracle(vr, gpu, golden, oracle):
    """Byte-for-byte: the voxel-window march, colmarch_kernel (vr_hip_set_column_copy(1)) and the CPU oracle, TRILINEAR and Q8, the
    column parity test's poses (flips at (180,90,0), reversed directions), 40x24x56 (march extents that are not multiples of 16)."""
    poses = ((0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (180.0, 90.0, 0.0), (0.0, 90.0, 0.0), (270.0, 0.0, 0.0), (0.0, 180.0, 0.0), (90.0, 90.0, 0.0), (0.0, 0.0, 90.0))
    taken = 0
    for name, label, sizes in (("bucky", "bench64_view1_default", ((256, 256), (130, 67))), ("blob_40x24x56", "view1_default", ((192, 160),))):
        st = golden.volume_state(name)
        gpu.set_transfer_fn(st["tf"], st["esl"])
        gpu.set_volume(golden.voxels(name))
        case = [c for c in golden.cases(True) if c["label"] == label and c["volume"] == name][0]
        for (w, h) in sizes:
            gpu.set_window_buffer(w, h)
            for angles in poses:
                for samp, kd, step_scale in ((vr.SAMPLE_TRILINEAR, 0.6, 1.0), (vr.SAMPLE_TRILINEAR_Q8, 0.0, 1.0), (vr.SAMPLE_TRILINEAR_Q8, 0.6, 0.37)):
                    p = _ortho(vr, golden, case, name, samp, w, h, angles, 2.0, kd, step_scale)
                    want = oracle.render(p, golden.voxels(name), st["tf"], st["esl"])
                    gpu.set_column_copy(0)
                    new = gpu.render_volume(p)
                    info = gpu.last_launch()
                    taken += info["column_voxels"]
                    gpu.set_column_copy(1)
                    old = gpu.render_volume(p)
                    assert gpu.last_launch()["column_voxels"] == 0
                    assert np.array_equal(new, old), (name, w, h, angles, samp, kd, step_scale)
                    assert np.array_equal(new, want), (name, w, h, angles, samp, kd, step_scale)
                    assert info["layout"] == 7 and info["column_voxels"] == 1, (name, angles, info)
    gpu.set_column_copy(0)
    assert taken > 0


@pytest.mark.gpu
def test_voxcol_policy_falls_back_when_the_rectangle_is_too_big(vr, gpu, golden, oracle):
    """The host takes the voxel windows only where (floor(7 * cells per pixel) + 4) per lateral axis multiply to <= 64; zoomed out
    to nearly one cell per pixel the frame falls back to colmarch_kernel (layout 7, column_voxels 0) — with the same image."""
    name, label = "bucky", "bench64_view1_default"
    st = golden.volume_state(name)
    gpu.set_transfer_fn(st["tf"], st["esl"])
    gpu.set_volume(golden.voxels(name))
    case = [c for c in golden.cases(True) if c["label"] == label and c["volume"] == name][0]
    dims = golden.voxels(name).shape[::-1]
    seen = set()
    for (w, zoom) in ((256, 2.0), (64, 2.0), (48, 2.0), (40, 2.0), (36, 2.0), (34, 2.0), (32, 2.0)):
        gpu.set_window_buffer(w, w)
        p = _ortho(vr, golden, case, name, vr.SAMPLE_TRILINEAR, w, w, (0.0, 0.0, 0.0), zoom, 0.6, 1.0)
        want = oracle.render(p, golden.voxels(name), st["tf"], st["esl"])
        img = gpu.render_volume(p)
        info = gpu.last_launch()
        assert np.array_equal(img, want), (w, zoom)
        if info["layout"] != 7:
            continue
        half = [np.float32(0.5) * np.float32(d) for d in dims]
        span = [math.floor(np.float32(7.0) * (abs(np.float32(p.view.right_plane[i])) + abs(np.float32(p.view.up_plane[i]))) * half[i]) + 4 for i in range(3)]
        m = info["brick_plane"]
        fits = span[1 if m == 0 else 0] * span[1 if m == 2 else 2] <= 64
        assert info["column_voxels"] == (1 if fits else 0), (w, zoom, span, info)
        seen.add(info["column_voxels"])
    assert seen == {0, 1}, seen
