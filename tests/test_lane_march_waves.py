"""scripts/lane_march_waves.py on the CPU: which waves of a column frame hold lanes that do not share kx bit for bit (col_wave_eligibility
sends them to the per-lane march).  The counts are those of the fp32 replay of pixel_ray / intersect, tile phase 0; the benchmark's view 3
and the custom pose (180,90,0) are the same camera."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from lane_march_waves import mixed_entry_waves, pixel_segments  # noqa: E402


@pytest.mark.parametrize("index", (0, 2))
def test_benchmark_views_0_and_2_have_no_mixed_entry_wave(vr, index):
    assert mixed_entry_waves(vr.benchmark_view(2048, 2048, index)) == []


def test_benchmark_view_3_has_one_row_of_mixed_entry_waves(vr):
    view = vr.benchmark_view(2048, 2048, 3)
    waves = mixed_entry_waves(view)
    assert len(waves) == 256 and {wy for _, wy, _ in waves} == {215}, (len(waves), sorted({wy for _, wy, _ in waves}))
    assert sorted(wx for wx, _, _ in waves) == list(range(256)) and {n for _, _, n in waves} == {2}
    kx, ky, alive = pixel_segments(view)
    assert alive.all() and (kx < ky).all()                        # the cube fills the frame: every lane of every wave is live


@pytest.mark.parametrize("viewport,count,row", ((64, 8, 6), (128, 16, 13)))
def test_small_viewports_of_the_same_pose(vr, viewport, count, row):
    waves = mixed_entry_waves(vr.custom_view(viewport, viewport, False, (180.0, 90.0, 0.0), 2.0))
    assert len(waves) == count and {wy for _, wy, _ in waves} == {row}, waves
