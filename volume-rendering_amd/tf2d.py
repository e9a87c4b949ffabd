"""Tf2dRenderer — the python face of the 2D transfer-function frames (include/vr_hip.h vr_hip_set_tf2d): a
HipRenderer whose composite frames can classify by value and gradient magnitude, and the histogram over both that places the table's rows.
A module of its own: HipRenderer's surface and the package's __all__ stay what they are."""
import ctypes as C

import numpy as np

from .renderer import HipRenderer, _ptr

TF_SIZE = 128


def _table(table):
    t = np.ascontiguousarray(table, dtype=np.float32)
    if t.ndim != 3 or t.shape[1:] != (TF_SIZE, 4):
        raise ValueError(f"a 2-D transfer function is (rows, {TF_SIZE}, 4) premultiplied floats, not {t.shape}")
    return t


def envelope(table):
    """The (128, 4) per-channel maximum over the rows of a (rows, 128, 4) table: a 1-D transfer function that is zero exactly where every
    row is.  Feed it to whatever builds the leaping bits of a 1-D function to get the bits set_tf2d takes."""
    return np.ascontiguousarray(_table(table).max(axis=0))


class Tf2dRenderer(HipRenderer):
    """HipRenderer with a table over (value, gradient magnitude).  The table is context state beside the 1-D transfer function: every other
    frame ignores it."""

    def set_tf2d(self, table, g_scale, esl=None):
        """table: (rows, 128, 4) premultiplied, 2..8 rows, row r a transfer function of the value; a sample of gradient magnitude g blends
        rows floor(g * g_scale) and the next.  esl: the 1024 leaping words built from envelope(table) — required, as for set_transfer_fn.
        Rows outside 2..8, a missing esl and members that are negative or not finite are the ABI's to refuse (VR_ERR_INVALID)."""
        t = _table(table)
        bits = None if esl is None else np.ascontiguousarray(esl, dtype=np.uint32)
        if bits is not None and bits.size != 1024:
            raise ValueError("esl holds 1024 words")
        self._check(self._L.vr_hip_set_tf2d(self._ctx, t.ctypes.data, t.shape[0], float(g_scale), None if bits is None else bits.ctypes.data), "set_tf2d")

    def clear_tf2d(self):
        self._check(self._L.vr_hip_set_tf2d(self._ctx, None, 0, 0.0, None), "clear_tf2d")

    def render_tf2d(self, params):
        """Host-buffer flavour: the composite frame classified by the 2-D table; an (out_rows, out_width, 4) uint8 array.  The context's
        clip, lighting and shadow apply; params.sampling must be one of the TRILINEAR modes."""
        return self._host_frame("render_tf2d", "vr_hip_render_tf2d", params, composite=True)

    def render_tf2d_device(self, params, dev_ptr, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None)."""
        self._frame("render_tf2d_device", "vr_hip_render_tf2d_device", params, C.c_void_p(dev_ptr), _ptr(stream), composite=True)

    def tf2d_frames(self):
        """vr_hip_tf2d_frames: the tf2d frames this context launched"""
        return self._counter("tf2d_frames", self._L.vr_hip_tf2d_frames)

    def gradient_histogram(self, g_bins, g_scale):
        """The (g_bins, 256) uint64 histogram of the resident volume over (gradient-magnitude row, value bin): row = round(g * g_scale)
        clamped to g_bins - 1.  The kernel's time in ms is left in last_gradient_histogram_ms."""
        h = np.empty((max(int(g_bins), 1), 256), dtype=np.uint64)       # (a count outside 1..32 is the ABI's to refuse: VR_ERR_INVALID)
        ms = C.c_float()
        self._check(self._L.vr_hip_gradient_histogram(self._ctx, int(g_bins), float(g_scale), h.ctypes.data, C.byref(ms)), "gradient_histogram")
        self.last_gradient_histogram_ms = float(ms.value)
        return h
