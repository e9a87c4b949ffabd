"""Test-side helpers of the 2D transfer-function tests: tf2d_render and gradient_histogram_ref of tests/tf2d_ref.c (the contract of
include/vr_hip.h vr_hip_render_tf2d / vr_hip_gradient_histogram restated with the CPU oracle's own statics on top of tests/feature_ref.c),
built through ref_library.compile_test_library; the tables both tiers use, their envelope, leaping bits and g-dependence flags; the choice
of g_scale per volume; and what the GPU tier does with one frame (check)."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY
from ref_library import Ref, SceneArgs, compile_test_library, contiguous, frame_array, ptr, volume_args

NEAREST_ROW, ROW_FROM_GG, NO_HALF, WEIGHT_Q8 = 1, 2, 3, 4       # the `perturb` of tf2d_render: the sensitivity test's wrong readings
PERTURBATIONS = (NEAREST_ROW, ROW_FROM_GG, NO_HALF, WEIGHT_Q8)
ROWS = 5                                                # the rows of the structured table
BAND = 16                                               # its entries alternate in bands of 16: rows equal to row 0, rows of their own


def envelope(table):
    """the per-channel maximum over the rows, stated here on its own (the package's tf2d.envelope is held to it)"""
    t = np.asarray(table, np.float32)
    out = t[0].copy()
    for row in t[1:]:
        out = np.where(row > out, row, out)
    return np.ascontiguousarray(out)


def g_dependent(table):
    """the 128 flags as four words: entry i is g-dependent unless every row holds row 0's bit patterns at i and at min(i + 1, 127)"""
    bits = np.ascontiguousarray(table, np.float32).view(np.uint32)
    same = np.array([all((bits[r, i] == bits[0, i]).all() for r in range(1, bits.shape[0])) for i in range(128)])
    words = np.zeros(4, np.uint32)
    for i in range(128):
        if not (same[i] and same[min(i + 1, 127)]):
            words[i >> 5] |= np.uint32(1 << (i & 31))
    return words


def dependent_entries(table):
    w = g_dependent(table)
    return np.array([(int(w[i >> 5]) >> (i & 31)) & 1 for i in range(128)], bool)


def esl_of(oracle, vox, table):
    """the leaping bits of a table: the reference's builder on the envelope (it reads the alpha channel alone) and the volume's block extrema"""
    return oracle.update_transfer_fn(envelope(table), oracle.volume_minmax(vox)[0])[1]


_tables = {}


def structured_table(tf):
    """Five rows from a volume's own premultiplied transfer function.  Entries alternate in bands of 16: in the even bands every row is row 0
    (g-independent but for each band's last entry, whose neighbour lies in the next band: 60 entries); in the odd bands row 0 is the
    function, row 1 the function at half its alpha (all four premultiplied channels halved: exact), row 2 zero, rows 3 and 4 a boundary
    colour ramp at alpha 1/4 and 1/2 (colours in 64ths: every member an exact float) — 68 g-dependent entries."""
    tf = np.ascontiguousarray(tf, np.float32).reshape(128, 4)
    key = tf.tobytes()
    if key not in _tables:
        t = np.repeat(tf[None], ROWS, axis=0).copy()
        for i in range(128):
            if (i // BAND) % 2 == 0:
                continue
            r = ((5 * i + 3) % 64) / 64.0
            t[1, i] = tf[i] * np.float32(0.5)
            t[2, i] = 0.0
            t[3, i] = (0.25 * r, 0.25 * 0.5, 0.25 * (1.0 - r), 0.25)
            t[4, i] = (0.5 * (1.0 - r), 0.5 * r, 0.5 * 0.75, 0.5)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def equal_rows(tf, rows=3):
    return np.ascontiguousarray(np.repeat(np.asarray(tf, np.float32).reshape(1, 128, 4), rows, axis=0))


def random_table(rng, tf):
    """2 to 8 rows drawn from `rng` around a scene's transfer function: row 0 is the function; every other row keeps it on a random third
    of the entries, scales it by a binary fraction on another third and is a random colour at a random alpha elsewhere"""
    tf = np.asarray(tf, np.float32).reshape(128, 4)
    rows = int(rng.integers(2, 9))
    t = np.repeat(tf[None], rows, axis=0).copy()
    kind = rng.integers(0, 3, size=128)
    for r in range(1, rows):
        scale = np.float32(rng.choice([0.0, 0.25, 0.5, 0.75]))
        alpha = rng.random(128).astype(np.float32) * (rng.random(128) < 0.6)
        colour = rng.random((128, 3)).astype(np.float32)
        t[r][kind == 1] = tf[kind == 1] * scale
        own = np.concatenate([colour * alpha[:, None], alpha[:, None]], axis=1).astype(np.float32)
        t[r][kind == 2] = own[kind == 2]
    return np.ascontiguousarray(t)


_library = None


def tf2d_library():
    """tests/tf2d_ref.c as a loaded library, built on first use"""
    global _library
    if _library is None:
        tmp = tempfile.mkdtemp(prefix="tf2d_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _library = compile_test_library(tmp, "tf2d_ref.c", "libtf2d_ref.so")
    return _library


class Tf2dFrame:
    """tf2d_render's answers for one frame: the frame, the samples of every pixel's accumulation loop, the samples with alpha by lower row,
    and by kind of entry (g-independent, g-dependent)"""

    def __init__(self, frame, count, by_row, by_kind):
        self.frame, self.count, self.by_row, self.by_kind = frame, count, by_row, by_kind


class Tf2dRef(Ref):
    """tf2d_render and gradient_histogram_ref of tests/tf2d_ref.c; frames cached per argument set."""

    def __init__(self):
        super().__init__()
        self.D = tf2d_library()
        self.D.tf2d_render.restype = C.c_int
        self.D.gradient_histogram_ref.restype = C.c_int

    def render(self, params, voxels, table, g_scale, esl, lighting=None, q=None, strength=1.0, clip=IDENTITY, perturb=0):
        t = contiguous(np.asarray(table), np.float32)
        assert t.ndim == 3 and t.shape[1:] == (128, 4)
        a = SceneArgs(params, voxels, t, esl, clip, lighting, q, strength)
        flags = g_dependent(t)

        def make():
            out, count = frame_array(params, 4), frame_array(params, dtype=np.uint32)
            by_row, by_kind = np.zeros(8, np.uint64), np.zeros(2, np.uint64)
            assert self.D.tf2d_render(*a.base, C.c_uint32(t.shape[0]), C.c_float(g_scale), a.esl, a.clip, *a.lighting, *a.shadow, ptr(flags),
                                      C.c_uint32(perturb), ptr(out), ptr(count), ptr(by_row), ptr(by_kind)) == 0
            return (Tf2dFrame(out, count, by_row, by_kind),)
        return self.cached(("tf2d",) + a.key + (t.shape[0], float(np.float32(g_scale)), int(perturb)), a.keep, make)[0]

    def histogram(self, voxels, g_bins, g_scale):
        vox, volume = volume_args(voxels)
        hist = np.zeros((g_bins, 256), np.uint64)
        assert self.D.gradient_histogram_ref(*volume, C.c_uint32(g_bins), C.c_float(g_scale), ptr(hist)) == 0
        return hist


_scales = {}


def choose_g_scale(name, vox):
    """g_scale of a volume, from gradient_histogram_ref alone: the power of two nearest to 4 / G, G the gradient magnitude a tenth of the
    voxels with a non-zero gradient exceed — rows 0 to 4 of the structured table then all lie inside the volume's own range.  Two passes of
    32 rows: the first over the largest magnitude any volume of this size can have, the second over the range the first found occupied."""
    if name not in _scales:
        ref = Tf2dRef.instance()
        z, y, x = vox.shape
        bound = float(np.iinfo(vox.dtype).max) * 0.5 * max(x, y, z) * 3.0 ** 0.5
        first = ref.histogram(vox, 32, 31.0 / bound).sum(axis=1)
        top = (int(np.nonzero(first)[0].max()) + 0.5) * bound / 31.0
        second = ref.histogram(vox, 32, 31.0 / top).sum(axis=1).astype(np.int64)
        moving = second.copy()
        moving[0] = 0                                    # (row 0: the flat voxels and the slowest slopes)
        if moving.sum() == 0:
            _scales[name] = 1.0
        else:
            tail = np.cumsum(moving[::-1])[::-1]            # voxels in row r or above
            r = int(np.nonzero(tail * 10 >= moving.sum())[0].max())
            _scales[name] = float(2.0 ** round(np.log2(4.0 / (max(r, 1) * top / 31.0))))
    return _scales[name]


# ---- what the GPU tier (tests/test_gpu_tf2d.py) does with one frame ----

def tf2d_launch(info):
    """what every tf2d frame's launch looks like: what a labelled frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


def check(gpu, ref, case, table, g_scale, esl):
    """the host entry point against tf2d_render: bytes; returns the restatement's answers.  The table is the caller's business."""
    want = ref.render(case.p, case.vox, table, g_scale, esl, case.lighting, case.q, case.strength, case.clip)
    got = gpu.render_tf2d(case.p)
    info = gpu.last_launch()
    wrong = int((got != want.frame).any(axis=-1).sum())
    assert wrong == 0, (case.what, wrong, info)
    assert tf2d_launch(info), (case.what, info)
    return want
