"""Test-side helpers of the fused-frame tests: fused_render of tests/fused_ref.c (the contract of include/vr_hip.h vr_hip_render_fused restated
with the CPU oracle's own statics on top of tests/feature_ref.c), built through ref_library.compile_test_library; the second field, its two
transfer functions and the leaping bits both tiers use; and what the GPU tier does with one frame (check)."""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np

from clip_helpers import IDENTITY
from ref_library import Ref, SceneArgs, compile_test_library, contiguous, frame_array, ptr

# the `perturb` of fused_render: the sensitivity test's wrong readings
B_CUE, WEIGHT_BEFORE_DENSE, B_IN_FRONT, TERMINATE_BETWEEN, SUM_TWO_FMAS, B_NEAREST = 1, 2, 3, 4, 5, 6
READINGS = {B_CUE: "B shaded with A's cue", WEIGHT_BEFORE_DENSE: "weight before A's dense test", B_IN_FRONT: "OVER with B in front",
            TERMINATE_BETWEEN: "OVER terminating between", SUM_TWO_FMAS: "SUM as two fmas", B_NEAREST: "B sampled nearest"}
MODE_OF = {B_CUE: "sum", WEIGHT_BEFORE_DENSE: "sum", B_IN_FRONT: "over", TERMINATE_BETWEEN: "over", SUM_TWO_FMAS: "sum", B_NEAREST: "over"}
MODES = {"sum": 0, "over": 1}
KINDS = ("none", "A only", "B only", "both")
INSIDE = (0.625, 0.4375)                                # the weight pair strictly inside (0, 1): binary fractions, so no product with them is special
HOT_ZEROS = 6                                           # leading all-zero entries of the hot ramp: both of B's shortcuts engage, below the 13-21 of the volumes' own
HOT_NOTCH = (48, 64)                                    # ... and a band of zero entries inside it: values only field A shows, even where B is A mirrored onto itself

_seconds = {}


def second_field(vox):
    """B for a volume A: A mirrored along x and z — the same dims and type, structures that cross A's and do not coincide"""
    key = (vox.ctypes.data, vox.shape)
    if key not in _seconds:
        b = np.ascontiguousarray(vox[::-1, :, ::-1])
        b.setflags(write=False)
        _seconds[key] = (b, vox)                        # (vox kept alive: its address is the key)
    return _seconds[key][0]


def hot_ramp(zeros=HOT_ZEROS, notch=HOT_NOTCH):
    """(128, 4) premultiplied: `zeros` leading all-zero entries, then black-red-yellow-white with alpha rising from 1/32 to 17/32, but for the
    zero entries [notch[0], notch[1]); zeros = 0 leaves no leading zero entry — the skip_mask 0 / skip_cmp 1 path of B's corner test"""
    t = np.zeros((128, 4), np.float32)
    for i in range(zeros, 128):
        if notch[0] <= i < notch[1]:
            continue
        u = (i - zeros) / float(127 - zeros)
        alpha = 1.0 / 32.0 + 0.5 * u
        t[i] = (min(1.0, 3.0 * u) * alpha, min(1.0, max(0.0, 3.0 * u - 1.0)) * alpha, min(1.0, max(0.0, 3.0 * u - 2.0)) * alpha, alpha)
    t.setflags(write=False)
    return t


HOT, HOT_OPEN = hot_ramp(), hot_ramp(0)


def bits_of(oracle, vox, tf):
    """the leaping bits of one field under one function: the reference's builder (it reads the alpha channel alone) on the volume's block extrema"""
    return oracle.update_transfer_fn(np.asarray(tf, np.float32).reshape(128, 4), oracle.volume_minmax(vox)[0])[1]


def fused_esl(bits_a, bits_b):
    """the AND, stated here on its own (the package's fusion.fused_esl is held to it)"""
    return np.ascontiguousarray(np.asarray(bits_a, np.uint32) & np.asarray(bits_b, np.uint32))


def fused_bits(oracle, case_esl, b, tf_b):
    return fused_esl(case_esl, bits_of(oracle, b, tf_b))


_library = None


def fused_library():
    """tests/fused_ref.c as a loaded library, built on first use"""
    global _library
    if _library is None:
        tmp = tempfile.mkdtemp(prefix="fused_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _library = compile_test_library(tmp, "fused_ref.c", "libfused_ref.so")
    return _library


class FusedFrame:
    """fused_render's answers for one frame: the frame, the samples of every pixel's accumulation loop, the samples by which field
    contributed (KINDS), and the accumulated floats the bytes are made of"""

    def __init__(self, frame, count, by_kind, acc):
        self.frame, self.count, self.by_kind, self.acc = frame, count, by_kind, acc


class FusedRef(Ref):
    """fused_render of tests/fused_ref.c on WHOLE frames; cached per argument set."""

    def __init__(self):
        super().__init__()
        self.D = fused_library()
        self.D.fused_render.restype = C.c_int

    def render(self, params, voxels, tf, esl, second, tf_b, mode="sum", weight_a=1.0, weight_b=1.0, lighting=None, q=None, strength=1.0, clip=IDENTITY, perturb=0):
        a = SceneArgs(params, voxels, tf, esl, clip, lighting, q, strength)
        b = contiguous(second)
        assert b.shape == np.asarray(voxels).shape and b.dtype == np.asarray(voxels).dtype
        tb = contiguous(np.asarray(tf_b), np.float32)
        m = MODES[mode] if isinstance(mode, str) else int(mode)

        def make():
            out, count, by_kind = frame_array(params, 4), frame_array(params, dtype=np.uint32), np.zeros(4, np.uint64)
            acc = frame_array(params, 4, dtype=np.float32)
            assert self.D.fused_render(*a.base, a.esl, a.clip, *a.lighting, *a.shadow, ptr(b), ptr(tb), C.c_uint32(m), C.c_float(weight_a), C.c_float(weight_b),
                                       C.c_uint32(perturb), ptr(out), ptr(count), ptr(by_kind), ptr(acc)) == 0
            return (FusedFrame(out, count, by_kind, acc),)
        key = ("fused",) + a.key + (b.ctypes.data, tb.tobytes(), m, float(np.float32(weight_a)), float(np.float32(weight_b)), int(perturb))
        return self.cached(key, a.keep + (b, tb), make)[0]


# ---- what the GPU tier (tests/test_gpu_fused.py) does with one frame ----

def acc_diff(a, b):
    """pixels whose accumulated floats differ in a bit"""
    return int((a.acc.view(np.uint32) != b.acc.view(np.uint32)).any(axis=-1).sum())


def fused_launch(info):
    """what every fused frame's launch looks like: what a labelled frame reads, tiles in grid order"""
    return info["layout"] in (0, 1, 5) and info["ordered"] == 0


def check(gpu, ref, case, second, tf_b, bits, mode="sum", weight_a=1.0, weight_b=1.0):
    """the host entry point against fused_render: bytes; returns the restatement's answers.  B, its function and the bits are the caller's business."""
    want = ref.render(case.p, case.vox, case.tf, bits, second, tf_b, mode, weight_a, weight_b, case.lighting, case.q, case.strength, case.clip)
    got = gpu.render_fused(case.p, weight_a, weight_b, mode)
    info = gpu.last_launch()
    wrong = int((got != want.frame).any(axis=-1).sum())
    assert wrong == 0, (case.what, mode, weight_a, weight_b, wrong, info)
    assert fused_launch(info), (case.what, info)
    return want
