"""The GPU feeders (minmax_kernel, histogram_kernel of csrc/vr_builders.hip; mip_bounds_kernel of csrc/vr_project.hip behind them) on every
path they have: the min/max scan's streaming path (8-deep unrolled loop, remainder loop, ragged last blocks, threads without a row, one
chunk per row), its chunked path (rows that are no power of two of chunks, more than 256 chunks) and its generic path, each for 1- and
2-byte voxels, and the histogram's 16-byte body with its tail of fewer than 16 bytes.

TABLE names, per shape, the path the kernel must take; scan_path restates the kernel's own conditions, and a CPU test holds the table
against it — a mirror, not a proof: it is there so that a change of the kernel's conditions makes someone revisit the table.

Two volumes per shape: noise over the dtype's whole range, and a BLOCK-CODED volume — every ESL block's values lie in a band of eight whose
position depends on (bx, by, bz), the band's lowest value at the block's first voxel and its highest at the block's last, so that a value
leaking in from a neighbouring block, or a row or chunk left out, changes that block's min or max.  2-byte voxels carry the band in the
high byte and an independent low byte: reading the wrong byte cannot pass by accident.

CPU tier: the oracle's scan and histogram equal a plain numpy construction.  GPU tier, byte for byte: the feeders equal that construction;
nothing of an earlier volume survives; the ESL bits built from the GPU scan equal those from the oracle's; MIP and isosurface frames that
skip by the block maxima derived from the scan equal the restatements of tests/feature_ref.c; and a leaping composite frame whose ESL bits
come from the GPU scan equals the oracle's frame."""
import numpy as np
import pytest

from iso_helpers import IsoRef, depth_bits, frame_params
from mip_helpers import MipRef, ramp_tf

gpu_test = pytest.mark.gpu

GRID = 32                  # VR_ESL_VOLUME_DIMS: blocks per axis of the ESL grid
MIN_BLOCK = 8              # VR_ESL_MIN_BLOCK
CHUNK = 16                 # bytes per load of the chunked paths and of the histogram's body

# ---- the shape table ---------------------------------------------------------------------------------------------------------------------
# (shape (z, y, x), bytes per voxel, block edge, path, chunks per row, facts).  facts: unrolled — the largest block has more than
# 7 * rows_per_pass rows, so the 8-deep loop runs (streaming rows say so either way); last_block — (rows along y, slices along z) of the
# ragged last block; idle — a pass has more row slots than the block has rows; tail, chunks — the histogram's tail bytes and whole chunks.
TABLE = (
    ((5, 40, 512), 1, 16, "streaming", 32, dict(unrolled=True, last_block=(8, 5))),
    ((2, 1000, 128), 1, 32, "streaming", 8, dict(unrolled=False, last_block=(8, 2))),
    ((3, 500, 16), 1, 16, "streaming", 1, dict(unrolled=False, idle=True, last_block=(4, 3))),
    ((3, 500, 48), 1, 16, "chunked", 3, dict()),
    ((2, 1000, 96), 1, 32, "chunked", 6, dict()),
    ((2, 3, 8192), 1, 256, "chunked", 512, dict()),
    ((9, 130, 17), 1, 8, "generic", 0, dict(tail=2)),
    ((2, 3, 5), 1, 8, "generic", 0, dict(tail=14, chunks=1)),
    ((1, 1, 1), 1, 8, "generic", 0, dict(tail=1, chunks=0)),
    ((20, 9, 256), 2, 8, "streaming", 32, dict(unrolled=True, last_block=(1, 4))),
    ((17, 40, 64), 2, 8, "streaming", 8, dict(unrolled=False, last_block=(8, 1))),
    ((3, 500, 64), 2, 16, "streaming", 8, dict(unrolled=False, last_block=(4, 3))),
    ((1, 1, 8), 2, 8, "streaming", 1, dict(unrolled=False, idle=True)),
    ((7, 9, 24), 2, 8, "chunked", 3, dict()),
    ((17, 40, 40), 2, 8, "chunked", 5, dict()),
    ((3, 500, 24), 2, 16, "chunked", 3, dict()),
    ((17, 40, 137), 2, 8, "generic", 0, dict()),
    ((3, 320, 16), 2, 10, "generic", 0, dict()),
    ((3, 5, 7), 2, 8, "generic", 0, dict(tail=2, chunks=13)),
    ((1, 1, 7), 2, 8, "generic", 0, dict(tail=14, chunks=0)),
)
KINDS = ("noise", "coded")


def row_id(row):
    (z, y, x), bpv = row[0], row[1]
    return f"{z}x{y}x{x}-{bpv}B"


ROWS = pytest.mark.parametrize("row", TABLE, ids=row_id)
# the shapes whose frames are rendered with the block maxima of the scan, and those of the leaping composite frame
RENDERED = tuple(r for r in TABLE if (r[0], r[1]) in (((5, 40, 512), 1), ((3, 500, 48), 1), ((7, 9, 24), 2), ((17, 40, 40), 2), ((20, 9, 256), 2)))
COMPOSITED = tuple(r for r in TABLE if (r[0], r[1]) in (((3, 500, 48), 1), ((17, 40, 40), 2)))


def block_edge(shape):
    return max(MIN_BLOCK, -(-max(shape) // GRID))


def scan_path(dim_x, bd, bpv):
    """minmax_kernel's path selection, restated: (path, chunks per row, rows per pass of the streaming path or None)"""
    chunk_voxels = CHUNK // bpv
    chunked = dim_x % chunk_voxels == 0 and bd % chunk_voxels == 0
    cpr = dim_x // chunk_voxels if chunked else 0
    if chunked and cpr <= 256 and (cpr & (cpr - 1)) == 0:
        return "streaming", cpr, 256 // cpr
    return ("chunked" if chunked else "generic"), cpr, None


def block_extents(n, bd):
    """voxels along one axis of every block: bd, and what is left for the last one"""
    return [min(bd, n - b0) for b0 in range(0, n, bd)]


# ---- the volumes -------------------------------------------------------------------------------------------------------------------------

def high_byte(vox):
    """what the ESL grid and the histogram see of a voxel"""
    return vox if vox.dtype == np.uint8 else (vox >> 8).astype(np.uint8)


def _with_low_byte(high, rng, bpv):
    if bpv == 1:
        return high
    return (high.astype(np.uint16) << 8) | rng.integers(0, 256, high.shape, dtype=np.uint16)


def noise_volume(shape, bpv, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256 ** bpv, shape, dtype=np.uint8 if bpv == 1 else np.uint16)


def band_base(bx, by, bz):
    return 8 + (7 * bx + 13 * by + 29 * bz) % 200


def coded_volume(shape, bpv, bd, seed):
    rng = np.random.default_rng(seed)
    z, y, x = shape
    high = np.zeros(shape, np.uint8)
    for bz in range(-(-z // bd)):
        for by in range(-(-y // bd)):
            for bx in range(-(-x // bd)):
                block = high[bz * bd:(bz + 1) * bd, by * bd:(by + 1) * bd, bx * bd:(bx + 1) * bd]
                block[...] = band_base(bx, by, bz) + rng.integers(0, 8, block.shape)
                block[0, 0, 0] = band_base(bx, by, bz)
                block[-1, -1, -1] = band_base(bx, by, bz) + 7
    return _with_low_byte(high, rng, bpv)


# ---- the plain references ----------------------------------------------------------------------------------------------------------------

def minmax_reference(vox, bd):
    """[bz, by, bx] -> (min, max) of the block's high bytes, one slice per block; {255, 0} where the grid holds no voxel"""
    s = high_byte(vox)
    z, y, x = s.shape
    out = np.empty((GRID, GRID, GRID, 2), np.uint8)
    out[..., 0], out[..., 1] = 255, 0
    for bz in range(-(-z // bd)):
        for by in range(-(-y // bd)):
            for bx in range(-(-x // bd)):
                block = s[bz * bd:(bz + 1) * bd, by * bd:(by + 1) * bd, bx * bd:(bx + 1) * bd]
                out[bz, by, bx] = block.min(), block.max()
    return out.reshape(-1, 2)


def histogram_reference(vox):
    return np.bincount(high_byte(vox).reshape(-1), minlength=256).astype(np.uint64)


_cases = {}


def case(row, kind):
    """(voxels, min/max reference, histogram reference) of a table row's volume of `kind`: built once, read-only"""
    key = (row[0], row[1], kind)
    if key not in _cases:
        shape, bpv, bd = row[0], row[1], row[2]
        seed = [20261020, TABLE.index(row), KINDS.index(kind)]
        vox = noise_volume(shape, bpv, seed) if kind == "noise" else coded_volume(shape, bpv, bd, seed)
        out = (vox, minmax_reference(vox, bd), histogram_reference(vox))
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


def holed_base_tf(oracle):
    """the default base transfer function with runs of 8 entries alternately transparent and opaque (an entry covers two voxel values, a
    coded block's band at most five entries): some coded blocks are empty, some are not"""
    base = oracle.default_base_tf()
    base[:, 3] = np.where((np.arange(128) // 8) % 2 == 1, np.float32(0.3), np.float32(0.0))
    return base


def empty_blocks(esl, shape, bd):
    """(empty, all) blocks of the grid the volume uses, from the ESL bits"""
    bits = ((np.asarray(esl, np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(GRID, GRID, GRID)
    used = bits[:-(-shape[0] // bd), :-(-shape[1] // bd), :-(-shape[2] // bd)]
    return int(used.sum()), int(used.size)


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------

@ROWS
def test_table_rows_land_on_the_path_they_name(row):
    shape, bpv, bd, path, cpr, facts = row
    z, y, x = shape
    assert bd == block_edge(shape)
    got_path, got_cpr, rows_per_pass = scan_path(x, bd, bpv)
    assert (got_path, got_cpr) == (path, cpr)
    ny, nz = block_extents(y, bd), block_extents(z, bd)
    if path == "streaming":
        assert (max(ny) * max(nz) > 7 * rows_per_pass) == facts["unrolled"]
        assert ("idle" in facts) == (max(ny) * max(nz) < rows_per_pass)
    else:
        assert "unrolled" not in facts and "idle" not in facts
    if "last_block" in facts:
        assert (ny[-1], nz[-1]) == facts["last_block"] and (ny[-1] < bd or nz[-1] < bd)
    size = z * y * x * bpv
    if "tail" in facts:
        assert size % CHUNK == facts["tail"] != 0
    else:
        assert size % CHUNK == 0
    if "chunks" in facts:
        assert size // CHUNK == facts["chunks"]
    assert z * y * x <= 256000


def test_the_table_reaches_every_path_for_both_widths():
    reached = {(bpv, path) for _, bpv, _, path, _, _ in TABLE}
    assert reached == {(b, p) for b in (1, 2) for p in ("streaming", "chunked", "generic")}
    for bpv in (1, 2):
        streaming = [r for r in TABLE if r[1] == bpv and r[3] == "streaming"]
        assert {r[5]["unrolled"] for r in streaming} == {True, False}
        assert any(r[4] == 1 for r in streaming) and any("last_block" in r[5] for r in streaming)
        tails = [r[5] for r in TABLE if r[1] == bpv and "tail" in r[5]]
        assert any(f.get("chunks", 1) == 0 for f in tails) and any(f.get("chunks", 1) > 0 for f in tails)
    assert any(r[4] > 256 for r in TABLE if r[3] == "chunked")
    assert any(r[2] % (CHUNK // r[1]) != 0 and r[0][2] % (CHUNK // r[1]) == 0 for r in TABLE if r[3] == "generic")     # the block edge alone


@ROWS
def test_oracle_scan_and_histogram_equal_numpy(oracle, row):
    shape, bpv, bd = row[0], row[1], row[2]
    for kind in KINDS:
        vox, mm, hist = case(row, kind)
        assert vox.shape == shape and vox.dtype.itemsize == bpv
        omm, obd, obs = oracle.volume_minmax(vox)
        assert obd == bd, kind
        assert np.array_equal(obs, np.array([np.float32(2.0) * np.float32(bd) / np.float32(n) for n in shape[::-1]], np.float32)), kind
        assert np.array_equal(omm, mm), kind
        assert np.array_equal(oracle.histogram(vox), hist) and int(hist.sum()) == vox.size, kind


@ROWS
def test_coded_volumes_carry_their_code(row):
    """every block holds its band's two ends, planted at its first and its last voxel, and the low bytes of 2-byte voxels are independent"""
    shape, bpv, bd = row[0], row[1], row[2]
    vox, mm, _ = case(row, "coded")
    s, grid = high_byte(vox), mm.reshape(GRID, GRID, GRID, 2)
    for bz, nz in enumerate(block_extents(shape[0], bd)):
        for by, ny in enumerate(block_extents(shape[1], bd)):
            for bx, nx in enumerate(block_extents(shape[2], bd)):
                lo = band_base(bx, by, bz)
                first, last = s[bz * bd, by * bd, bx * bd], s[bz * bd + nz - 1, by * bd + ny - 1, bx * bd + nx - 1]
                if nz * ny * nx > 1:
                    assert (first, last) == (lo, lo + 7) and tuple(grid[bz, by, bx]) == (lo, lo + 7), (bx, by, bz)
                else:
                    assert first == lo + 7 and tuple(grid[bz, by, bx]) == (lo + 7, lo + 7)
    if bpv == 2 and vox.size >= 1000:
        low = (vox & 0xff).astype(np.float64).reshape(-1)
        assert len(np.unique(low)) > 200 and abs(np.corrcoef(low, s.astype(np.float64).reshape(-1))[0, 1]) < 0.1


def test_holed_transfer_function_empties_some_coded_blocks(oracle):
    base = holed_base_tf(oracle)
    for row in COMPOSITED:
        _, mm, _ = case(row, "coded")
        empty, used = empty_blocks(oracle.update_transfer_fn(base, mm)[1], row[0], row[2])
        assert 0 < empty < used, (row_id(row), empty, used)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------

def assert_minmax(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        e = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} blocks differ, first (bx, by, bz) = {(e % GRID, e // GRID % GRID, e // (GRID * GRID))}: "
                             f"{tuple(got[e])} for {tuple(want[e])}")


@gpu_test
@ROWS
def test_scan_equals_numpy(gpu, oracle, row):
    for kind in KINDS:
        vox, mm, _ = case(row, kind)
        gpu.set_volume(vox)
        got, bd, bs, _ = gpu.volume_minmax()
        _, obd, obs = oracle.volume_minmax(vox)
        assert bd == obd == row[2] and np.array_equal(np.array(bs, np.float32), obs), (kind, bd, bs)
        assert got.shape == (GRID ** 3, 2)
        assert_minmax(got, mm, (row_id(row), kind))


@gpu_test
@ROWS
def test_histogram_equals_numpy(gpu, row):
    for kind in KINDS:
        vox, _, hist = case(row, kind)
        gpu.set_volume(vox)
        got, _ = gpu.volume_histogram()
        assert int(got.sum()) == vox.size, (kind, int(got.sum()))
        assert np.array_equal(got, hist), (kind, np.flatnonzero(got != hist)[:8])


@gpu_test
@pytest.mark.parametrize("first,second", ((((5, 40, 512), 1), ((2, 3, 5), 1)), (((3, 500, 48), 1), ((7, 9, 24), 2))), ids=("large-then-small", "1B-then-2B"))
def test_nothing_of_the_volume_before_survives(gpu, first, second):
    a, b = (next(r for r in TABLE if (r[0], r[1]) == which) for which in (first, second))
    for kind in KINDS:
        vox_a, mm_a, hist_a = case(a, kind)
        gpu.set_volume(vox_a)
        assert_minmax(gpu.volume_minmax()[0], mm_a, (row_id(a), kind))
        assert np.array_equal(gpu.volume_histogram()[0], hist_a)
        vox_b, mm_b, hist_b = case(b, kind)
        gpu.set_volume(vox_b)
        got = gpu.volume_minmax()[0]
        assert_minmax(got, mm_b, (row_id(b), kind, "after", row_id(a)))
        grid = got.reshape(GRID, GRID, GRID, 2).copy()
        grid[:-(-b[0][0] // b[2]), :-(-b[0][1] // b[2]), :-(-b[0][2] // b[2])] = (255, 0)
        assert (grid[..., 0] == 255).all() and (grid[..., 1] == 0).all()           # the blocks the second volume does not use
        hist = gpu.volume_histogram()[0]
        assert int(hist.sum()) == vox_b.size and np.array_equal(hist, hist_b), (kind, int(hist.sum()))


@gpu_test
@ROWS
def test_esl_bits_from_the_scan_equal_the_oracles(gpu, oracle, row):
    for kind in KINDS:
        vox, mm, _ = case(row, kind)
        gpu.set_volume(vox)
        got = gpu.volume_minmax()[0]
        for name, base in (("default", oracle.default_base_tf()), ("holed", holed_base_tf(oracle))):
            tf, esl = oracle.update_transfer_fn(base, got)
            otf, oesl = oracle.update_transfer_fn(base, oracle.volume_minmax(vox)[0])
            assert np.array_equal(esl, oesl) and np.array_equal(tf, otf), (kind, name, int((esl != oesl).sum()))


def _views(vr):
    """benchmark views 0, 2 and 3 look along one volume axis each, view 1 is the oblique orthogonal one; all at distance 2, where the host
    keeps skipping on (fetch_coordinates_exact of vr_hip_api.cpp: (1 + 2 max|origin|) * max_dim < 2^20)"""
    views = [(i, vr.benchmark_view(48, 40, i)) for i in range(4)]
    major = [int(np.argmax(np.abs(np.array(list(v.direction))))) for _, v in views]
    assert sorted(major[i] for i in (0, 2, 3)) == [0, 1, 2] and min(abs(d) for d in views[1][1].direction) > 0.3
    assert all(v.perspective == 0 and (1.0 + 2.0 * max(abs(o) for o in v.origin)) * 512 < 2 ** 20 for _, v in views)
    return views


def iso_level(vox):
    """the middle of the volume's coded range, in raw voxel units: bands below it, bands above it"""
    s = high_byte(vox)
    return ((int(s.min()) + int(s.max())) // 2 + 0.5) * (1 if vox.dtype == np.uint8 else 256)


def _diff(a, b):
    return int((a != b).any(axis=-1).sum())


@gpu_test
@pytest.mark.parametrize("row", RENDERED, ids=row_id)
def test_frames_skipping_by_the_scans_maxima_equal_the_restatements(vr, gpu, oracle, row):
    """MIP (NEAREST, TRILINEAR) and isosurface frames of the block-coded volume with esl off and on: a block maximum that is too low, in
    the scan or in the dilation behind it, skips samples these frames need"""
    vox, _, _ = case(row, "coded")
    tf = ramp_tf()
    level = iso_level(vox)
    gpu.set_window_buffer(128, 128)
    gpu.set_transfer_fn(tf, np.zeros(1024, np.uint32))
    gpu.set_volume(vox)
    covered = hits = 0
    for index, view in _views(vr):
        for sampling in (vr.SAMPLE_NEAREST, vr.SAMPLE_TRILINEAR):
            ref = MipRef.instance().render(frame_params(vr, oracle, vox, view, sampling, 0), vox, tf)[0]
            covered += int((ref[..., 3] != 0).sum())
            for esl in (0, 1):
                out = gpu.render_mip(frame_params(vr, oracle, vox, view, sampling, esl))
                assert _diff(out, ref) == 0, ("mip", index, sampling, esl, _diff(out, ref))
        ref = IsoRef.instance().render(frame_params(vr, oracle, vox, view, vr.SAMPLE_TRILINEAR, 0), vox, tf, level, 4)
        hits += ref[2]["hits"]
        for esl in (0, 1):
            out, depth = gpu.render_iso(frame_params(vr, oracle, vox, view, vr.SAMPLE_TRILINEAR, esl), level, 4, depth=True)
            wrong = int((depth_bits(depth) != depth_bits(ref[1])).sum())
            assert _diff(out, ref[0]) == 0 and wrong == 0, ("iso", index, esl, _diff(out, ref[0]), wrong)
    assert covered > 4000 and hits > 500, (covered, hits)       # the frames look at the volume, and at a surface


@gpu_test
@pytest.mark.parametrize("row", COMPOSITED, ids=row_id)
def test_leaping_composite_frame_from_the_gpu_scan(vr, gpu, oracle, row):
    """what an application does: min/max on the GPU, ESL bits from it, a frame that leaps by them — against the oracle's frame with the
    ESL bits of the oracle's own scan"""
    vox, _, _ = case(row, "coded")
    base = holed_base_tf(oracle)
    gpu.set_window_buffer(128, 128)
    gpu.set_volume(vox)
    mm, bd, bs, _ = gpu.volume_minmax()
    tf, esl = oracle.update_transfer_fn(base, mm)
    gpu.set_transfer_fn(tf, esl)
    otf, oesl, obd, obs, ray_step = oracle.scene_for(vox, base)
    p = vr.VrParams()
    p.view = vr.benchmark_view(48, 40, 1)
    p.ray_step, p.ray_threshold, p.light_kd = float(ray_step), 0.95, 0.6
    p.esl, p.esl_block_dims, p.sampling = 1, bd, vr.SAMPLE_TRILINEAR
    for j in range(3):
        p.esl_block_size[j] = bs[j]
    p = vr.whole_frame(p)
    assert bd == obd and np.array_equal(np.array(bs, np.float32), obs)
    out = gpu.render_volume(p)
    ref = oracle.render(p, vox, otf, oesl, threads=4)
    assert _diff(out, ref) == 0, _diff(out, ref)
    empty, used = empty_blocks(esl, row[0], row[2])
    assert 0 < empty < used and int((ref[..., 3] != 0).sum()) > 500, (empty, used)
