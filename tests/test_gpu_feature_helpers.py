"""tests/gpu_feature.py on the CPU: the walk of sweep_paths and what it leaves behind, the calls of reset_context, the rows of
expected_bands against the product's own band map, and MAPPINGS — on a stand-in that records every set_* / clear_* call"""
import ctypes as C

import numpy as np
import pytest

import gpu_feature as gf


class FakeVr:
    LAYOUT_BRICKED, LAYOUT_LINEAR = 0, 1


DEFAULTS = {"layout": FakeVr.LAYOUT_BRICKED, "brick_plane": -1, "wide_addressing": 0, "tile_mapping": (-1,), "tile_scheduling": 1}
RESTORE = [("set_tile_scheduling", 1), ("set_tile_mapping", -1), ("set_wide_addressing", 0), ("set_brick_plane", -1), ("set_layout", FakeVr.LAYOUT_BRICKED)]
WALK = ([("layout", 1), ("layout", 1, "wide"), ("layout", 0)] + [("plane", n) for n in range(-1, 10)] + [("wide", w) for w in (0, 1, 2, 4)] +
        [("mapping", o, s, ph) for o in range(3) for s in range(3) for ph in ((0, 0), (3, 5))] + [("scheduling", m) for m in (0, 1, 2)])
SHORT_WALK = [w for w in WALK if w not in (("layout", 1, "wide"), ("wide", 4)) and w[0] != "scheduling"]      # what the three keyword arguments leave out


class Recorder:
    """logs every set_* / clear_* call and keeps the last value of each knob"""

    def __init__(self):
        self.calls, self.state = [], dict(DEFAULTS)

    def __getattr__(self, name):
        if not name.startswith(("set_", "clear_")):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name,) + args)
            if name.startswith("set_"):
                self.state[name[4:]] = args if name == "set_tile_mapping" else args[0]
        return call


def knobs_of(what):
    """the state a step of sweep_paths promises its check: that step's knob, every other at its default"""
    kind, value = what[0], what[1:]
    if kind == "layout":
        return dict(DEFAULTS, layout=value[0], wide_addressing=int(value[1:] == ("wide",)))
    if kind == "mapping":
        order, shape, phase = value
        return dict(DEFAULTS, tile_mapping=(order + 4 * shape,) + phase)
    return dict(DEFAULTS, **{{"plane": "brick_plane", "wide": "wide_addressing", "scheduling": "tile_scheduling"}[kind]: value[0]})


@pytest.mark.parametrize("kwargs,want", (({}, WALK), (dict(linear_wide=False, wides=(0, 1, 2), schedulings=()), SHORT_WALK)), ids=("defaults", "short_walk"))
def test_sweep_paths_walks_one_knob_at_a_time(kwargs, want):
    gpu, seen = Recorder(), []

    def check(what):
        assert gpu.state == knobs_of(what), (what, gpu.state)
        seen.append(what)
    assert gf.sweep_paths(FakeVr, gpu, check, **kwargs) == want == seen
    assert len(want) == (34 if kwargs else 39)
    assert gpu.state == DEFAULTS and gpu.calls[-5:] == RESTORE


@pytest.mark.parametrize("fail_at", (0, 1, 2, 7, 14, 20, 35, 38))
def test_sweep_paths_restores_the_defaults_when_a_check_raises(fail_at):
    gpu, seen = Recorder(), []

    def check(what):
        seen.append(what)
        if len(seen) == fail_at + 1:
            raise AssertionError(what)
    with pytest.raises(AssertionError) as e:
        gf.sweep_paths(FakeVr, gpu, check)
    assert e.value.args == (WALK[fail_at],) and seen == WALK[:fail_at + 1]
    assert gpu.state == DEFAULTS and gpu.calls[-5:] == RESTORE


def test_reset_context_makes_all_nine_calls():
    gpu = Recorder()
    gf.reset_context(FakeVr, gpu)
    assert gpu.calls == [("clear_preintegration",), ("clear_lighting",), ("clear_shadow",), ("clear_clip",), ("set_layout", FakeVr.LAYOUT_BRICKED),
                         ("set_tile_mapping", -1), ("set_tile_scheduling", 1), ("set_wide_addressing", 0), ("set_brick_plane", -1)]


@pytest.mark.parametrize("rank,world,band_rows,height", ((1, 3, 16, 72), (1, 3, 16, 80), (0, 2, 3, 70), (1, 2, 3, 70)))
def test_expected_bands_is_the_products_band_map(vr, rank, world, band_rows, height):
    """vr.band_partition's geometry (vr_hip_multi_band_map, a host function of the C ABI): frame row y is row local_row of its rank's buffer"""
    L = vr.lib()
    whole = np.arange(height * 5 * 4, dtype=np.uint8).reshape(height, 5, 4) | 1          # no row of zeros
    p = vr.VrParams()
    p.view = vr.benchmark_view(5, height, 0)
    rows = vr.band_partition(p, rank, world, band_rows)[0].out_rows
    out = gf.expected_bands(whole, rank, world, band_rows, rows)
    assert out.shape == (rows, 5, 4) and out.dtype == whole.dtype
    held = np.zeros(rows, bool)
    for y in range(height):
        owner, local_row = C.c_uint32(), C.c_uint32()
        L.vr_hip_multi_band_map(world, band_rows, y, C.byref(owner), C.byref(local_row))
        if owner.value == rank:
            assert np.array_equal(out[local_row.value], whole[y]), y
            held[local_row.value] = True
    assert np.array_equal(out.any(axis=(1, 2)), held) and held.any()                      # rows beyond the frame are zero
    assert held.all() == ((rank, height) in ((1, 80), (0, 70)))
    depth = gf.expected_bands(np.ones((height, 5), np.float32), rank, world, band_rows, rows, beyond=-1)
    assert (depth[held] == 1).all() and (depth[~held] == -1).all()


def test_mappings():
    assert len(gf.MAPPINGS) == len(set(gf.MAPPINGS)) == 18
    assert {m for m, _ in gf.MAPPINGS} == {o + 4 * s for o in range(3) for s in range(3)} and {ph for _, ph in gf.MAPPINGS} == {(0, 0), (3, 5)}
    assert gf.PLANES == tuple(range(-1, 10)) and gf.WIDES == (0, 1, 2, 4) and gf.SCHEDULINGS == (0, 1, 2)
