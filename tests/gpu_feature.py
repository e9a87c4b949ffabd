"""What the GPU tiers of the render features (tests/test_gpu_{mip,iso,clip,shadow,light,slab,backdrop,section,feature_random}.py) share,
stated once: the frame comparisons, the loader and the reset of the session's context, the walk over every placement and addressing path,
the repeated frame under the measured-cost tile order, the rows of a band-partitioned frame, the child run under the bounds-checked
build, the two-context MultiRenderer and the volr_bench run.  What is compared, and the message of a failure, stay with each file."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN_DIR, ROOT
from iso_helpers import depth_bits


def diff(a, b):
    """pixels that differ"""
    return int((a != b).any(axis=-1).sum())


def depth_diff(a, b):
    """depths that differ in a bit"""
    return int((depth_bits(a) != depth_bits(b)).sum())


def load(gpu, vox, tf, esl=None, window=(128, 128)):
    """esl None: no block is empty (the ESL bits a MIP or an isosurface frame is given are unused)"""
    gpu.set_window_buffer(*window)
    gpu.set_transfer_fn(tf, np.zeros(1024, np.uint32) if esl is None else esl)
    gpu.set_volume(vox)


def reset_context(vr, gpu):
    """every state and every forced path of the context back to its default"""
    gpu.clear_preintegration()
    gpu.clear_lighting()
    gpu.clear_shadow()
    gpu.clear_clip()
    gpu.set_layout(vr.LAYOUT_BRICKED)
    gpu.set_tile_mapping(-1)
    gpu.set_tile_scheduling(1)
    gpu.set_wide_addressing(0)
    gpu.set_brick_plane(-1)


# ---- every path agrees ---------------------------------------------------------------------------------------------------------------

PLANES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9)      # vr_hip_set_brick_plane: the context's choice, and each copy forced
WIDES = (0, 1, 2, 4)                             # vr_hip_set_wide_addressing: 32-bit tables, 64-bit tables, index arithmetic, +4
MAPPINGS = tuple((order + 4 * shape, phase) for order in range(3) for shape in range(3) for phase in ((0, 0), (3, 5)))    # (lane_map, phase)
SCHEDULINGS = (0, 1, 2)
PATH_VOLUMES = (("blob_40x24x56", {0, 1}), ("random_u16", {0, 1, 5}))        # (volume, the layouts its frames are launched on): u8, u16 (oct bricks)


def sweep_paths(vr, gpu, check, linear_wide=True, wides=WIDES, schedulings=SCHEDULINGS):
    """Placement and addressing only.  check(what) runs once per step with that step's knob set and every other at its default: linear /
    bricked (and, with linear_wide, the linear array under 64-bit tables between them), for plane in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9) the
    forced brick plane, `wides`, every lane order x wave shape x two phases of MAPPINGS, `schedulings`.  Whatever check raises, the context
    is left on its defaults.  Returns the `what` of every step that ran."""
    ran = []

    def step(*what):
        check(what)
        ran.append(what)
    try:
        for layout in (vr.LAYOUT_LINEAR, vr.LAYOUT_BRICKED):
            gpu.set_layout(layout)
            step("layout", layout)
            if linear_wide and layout == vr.LAYOUT_LINEAR:
                gpu.set_wide_addressing(1)
                step("layout", layout, "wide")
                gpu.set_wide_addressing(0)
        for plane in PLANES:
            gpu.set_brick_plane(plane)
            step("plane", plane)
        gpu.set_brick_plane(-1)
        for wide in wides:
            gpu.set_wide_addressing(wide)
            step("wide", wide)
        gpu.set_wide_addressing(0)
        for lane_map, phase in MAPPINGS:
            gpu.set_tile_mapping(lane_map, *phase)
            step("mapping", lane_map % 4, lane_map // 4, phase)
        gpu.set_tile_mapping(-1)
        for mode in schedulings:
            gpu.set_tile_scheduling(mode)
            step("scheduling", mode)
    finally:
        gpu.set_tile_scheduling(1)
        gpu.set_tile_mapping(-1)
        gpu.set_wide_addressing(0)
        gpu.set_brick_plane(-1)
        gpu.set_layout(vr.LAYOUT_BRICKED)
    return ran


def assert_order_repeats(gpu, render, want, times=4, min_ordered=3, what=()):
    """render() `times` times under the measured-cost tile order: every frame equals `want`, and at least min_ordered of them started
    their tiles in a recorded order (the first frame runs in the estimated order or in none)"""
    ordered = 0
    for k in range(times):
        out = render()
        assert diff(out, want) == 0, (*what, k, diff(out, want), gpu.last_launch())
        ordered += gpu.last_launch()["ordered"]
    assert ordered >= min_ordered, (*what, ordered)


def expected_bands(want, rank, world, band_rows, rows, beyond=0):
    """The `rows` rows that rank `rank` of `world` holds of the frame `want` under interleaved bands of band_rows rows: local row ly is
    frame row ((ly // band_rows) * world + rank) * band_rows + ly % band_rows, and `beyond` (zeros) past the frame's height"""
    ly = np.arange(rows)
    gy = ((ly // band_rows) * world + rank) * band_rows + ly % band_rows
    inside = gy < want.shape[0]
    out = np.full((rows,) + want.shape[1:], beyond, want.dtype)
    out[inside] = want[gy[inside]]
    return out


# ---- child processes --------------------------------------------------------------------------------------------------------------------

BOUNDS_LIB = os.path.join(ROOT, "build_variants", "libvr_hip_bounds.so")
needs_bounds_lib = pytest.mark.skipif(not os.path.exists(BOUNDS_LIB),
                                      reason="build_variants/libvr_hip_bounds.so not built (scripts/build_variant.sh bounds -DVR_BOUNDS_CHECK)")


def run_under_bounds_build(test_file, k, passed, timeout):
    """The GPU tests of test_file that `-k` selects, once in a child process with the -DVR_BOUNDS_CHECK library (tests/test_gpu_bounds.py):
    every gather address is held against its array — a violation fails the frame (VrError) — and exactly `passed` tests pass"""
    env = dict(os.environ, VR_HIP_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(test_file), "-m", "gpu", "-x", "-q", "-k", k],
                       capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0 and f"{passed} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@contextlib.contextmanager
def multi_pair(vr, monkeypatch, transport, window=(120, 72)):
    """MultiRenderer([0, 0]) — two contexts on one device — over `transport` ("peer": peer copies, "rccl-self": RCCL with one
    communicator), checking itself, with its window set; closed on the way out"""
    monkeypatch.setenv("VR_MULTI_TRANSPORT", transport)
    monkeypatch.setenv("VR_MULTI_SELFCHECK", "1")
    m = vr.MultiRenderer([0, 0])
    try:
        assert m.transport == ("peer-copy" if transport == "peer" else "rccl-self")
        m.set_window_buffer(*window)
        yield m
    finally:
        m.close()


def run_driver(tmp_path, *flags, size=(256, 256), pose=("-45", "-45", "0", "2"), renderer="1", output="frame.ppm"):
    """volr_bench -f Bucky.pvm -r renderer -s size <flags> -pose ... -o tmp_path/output; a None leaves that option out.  Returns the
    completed process and the frame it wrote as (h, w, 3) rows from the top, or None where it failed or wrote none."""
    line = [os.path.join(ROOT, "volume-rendering_amd", "volr_bench"), "-f", os.path.join(GOLDEN_DIR, "Bucky.pvm")]
    line += [] if renderer is None else ["-r", renderer]
    line += ["-s", str(size[0]), str(size[1]), *flags]
    line += [] if pose is None else ["-pose", *pose]
    line += [] if output is None else ["-o", str(tmp_path / output)]
    out = subprocess.run(line, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 or output is None:
        return out, None
    header = b"P6\n%d %d\n255\n" % size
    data = (tmp_path / output).read_bytes()
    assert data.startswith(header), data[:32]
    return out, np.frombuffer(data[len(header):], np.uint8).reshape(size[1], size[0], 3)[::-1]
