"""The one loader of the CPU restatements: tests/feature_ref.c (every render feature of include/vr_hip.h restated with the CPU oracle's own
statics) and tests/mip_bound_ref.c (the MIP's skip bound checked per sample), compiled once per session into a temporary directory with
the flags oracle/Makefile uses for libvr_oracle.so; the marshalling of the arguments their entry points share; and the base of the seven
*Ref classes of tests/*_helpers.py, which keep one instance each and cache their read-only results per argument set."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what oracle/Makefile builds libvr_oracle.so with
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-fopenmp"]


def compile_test_library(tmp_dir, source, name):
    lib = os.path.join(tmp_dir, name)
    subprocess.check_call(["gcc", *CFLAGS, "-o", lib, os.path.join(ROOT, "tests", source), "-lm"])
    return C.CDLL(lib)


_libraries = None


def libraries():
    """(tests/feature_ref.c, tests/mip_bound_ref.c) as loaded libraries, built on first use"""
    global _libraries
    if _libraries is None:
        tmp = tempfile.mkdtemp(prefix="ref_library_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _libraries = (compile_test_library(tmp, "feature_ref.c", "libfeature_ref.so"), compile_test_library(tmp, "mip_bound_ref.c", "libmip_bound_ref.so"))
    return _libraries


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def contiguous(a, dtype=None):
    """`a` itself where it can be passed as it is: results are cached by the address of the voxels"""
    return a if a.flags["C_CONTIGUOUS"] and dtype in (None, a.dtype) else np.ascontiguousarray(a, dtype=dtype)


def volume_args(voxels):
    """(voxels, [voxels, dims, bytes per voxel] as the entry points take them)"""
    vox = contiguous(voxels)
    z, y, x = vox.shape
    return vox, [ptr(vox), (C.c_uint32 * 3)(x, y, z), C.c_uint32(vox.dtype.itemsize)]


def clip_floats(clip):
    """the ten floats of vr_clip"""
    box_min, box_max, plane = clip
    return np.array(list(box_min or (-1, -1, -1)) + list(box_max or (1, 1, 1)) + list(plane or (0, 0, 0, 0)), np.float32)


def frame_array(params, *tail, dtype=np.uint8):
    return np.zeros((params.out_rows, params.out_width) + tail, dtype)


class SceneArgs:
    """The arguments the entry points of tests/feature_ref.c share, marshalled once, for a WHOLE frame.
    base: params, voxels, dims, bytes per voxel, tf — what every entry point begins with;
    esl, clip: pointers (None where not given);
    shadow: q, S, strength;  lighting: the three coefficients, shininess_log2 (None, 0: the reference's cue);  mode: the classification;
    key: all of it, for the cache;  keep: the arrays behind the pointers and the key's addresses."""

    def __init__(self, params, voxels, tf, esl=None, clip=None, lighting=None, q=None, strength=1.0, mode=0):
        assert params.x0 == 0 and params.out_width == params.view.width and params.out_rows == params.view.height and params.band_stride == 1
        vox, volume = volume_args(voxels)
        tf = contiguous(np.asarray(tf), np.float32)
        esl = None if esl is None else contiguous(np.asarray(esl), np.uint32)
        cf = None if clip is None else clip_floats(clip)
        lf = None if lighting is None else np.array(lighting[:3], np.float32)
        shin = 0 if lighting is None else int(lighting[3])
        qq = None if q is None else contiguous(q)
        self.base = [C.byref(params), *volume, ptr(tf)]
        self.esl, self.clip = ptr(esl), ptr(cf)
        self.lighting = [ptr(lf), C.c_uint32(shin)]
        self.shadow = [ptr(qq), C.c_uint32(0 if qq is None else qq.shape[0]), C.c_float(strength)]
        self.mode = C.c_uint32(mode)
        self.key = (bytes(params), vox.ctypes.data, vox.shape, tf.tobytes()) + tuple(None if a is None else a.tobytes() for a in (esl, cf, lf, qq)) + \
                   (shin, float(np.float32(strength)), int(mode))
        self.keep = (vox, tf, esl, cf, lf, qq)


class Ref:
    """Base of MipRef, IsoRef, ClipRef, ShadowRef, LightRef, SlabRef and BackdropRef: one instance per class, all on the one library."""
    _instances = {}

    @classmethod
    def instance(cls):
        if cls not in Ref._instances:
            Ref._instances[cls] = cls()
        return Ref._instances[cls]

    def __init__(self):
        self.L, self.B = libraries()
        self._cache = {}

    def cached(self, key, keep, make):
        """make() -> a tuple of results, computed once per key; its arrays are made read-only, and `keep` (the arrays whose addresses are part
        of the key or behind the call's pointers) stays alive with it"""
        if key not in self._cache:
            out = make()
            for a in out:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._cache[key] = (out, keep)
        return self._cache[key][0]
