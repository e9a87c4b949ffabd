"""FusedRenderer — the python face of the fused frames (include/vr_hip.h vr_hip_render_fused): a HipRenderer whose
composite frames can show a second, co-registered field with a transfer function of its own, weighted against the resident one in one
march.  A module of its own: HipRenderer's surface and the package's __all__ stay what they are."""
import ctypes as C

import numpy as np

from .binding import VrError, make_fusion
from .renderer import HipRenderer, _ptr

_TORCH_DTYPES = {"torch.uint8": 1, "torch.uint16": 2, "torch.int16": 2}


def fused_esl(bits_a, bits_b):
    """The leaping bits of a fused frame: a block may be leapt only where it is empty in BOTH fields — the AND of field A's bits under A's
    transfer function and field B's bits under B's, 1024 words each."""
    a = np.ascontiguousarray(bits_a, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(bits_b, dtype=np.uint32).reshape(-1)
    if a.size != 1024 or b.size != 1024:
        raise ValueError("esl holds 1024 words")
    return np.ascontiguousarray(a & b)


class FusedRenderer(HipRenderer):
    """HipRenderer with a second field.  The field, its transfer function and the fused frame's leaping bits are context state beside the
    resident volume: every other frame ignores them.  A new volume drops the field; its function and the bits stay."""

    def set_second_volume(self, voxels):
        """vr_hip_set_second_volume: field B, with the dims and the dtype of the resident volume.  `voxels` is a numpy array shaped (z, y, x)
        of uint8 or uint16, or a contiguous device tensor of that shape (1 or 2 bytes per element; copied on the context's stream).  Other
        dims or another voxel size are the ABI's to refuse (VR_ERR_INVALID)."""
        if hasattr(voxels, "data_ptr"):
            size = _TORCH_DTYPES.get(str(voxels.dtype))
            if size is None or voxels.dim() != 3 or not voxels.is_contiguous() or not voxels.is_cuda:
                raise VrError(1, "the second volume must be a contiguous 3-D device tensor of 1- or 2-byte integers")
            z, y, x = (int(n) for n in voxels.shape)
            self._check(self._L.vr_hip_set_second_volume_device(self._ctx, C.c_void_p(voxels.data_ptr()), x, y, z, size), "set_second_volume")
            return
        v = np.ascontiguousarray(voxels)
        if v.dtype not in (np.uint8, np.uint16) or v.ndim != 3:
            raise VrError(1, "the second volume must be a 3-D uint8 / uint16 array")
        z, y, x = v.shape
        self._check(self._L.vr_hip_set_second_volume(self._ctx, v.ctypes.data, x, y, z, v.dtype.itemsize), "set_second_volume")

    def clear_second_volume(self):
        """Drops field B: render_fused is VR_ERR_NOT_READY until it is set again.  Its transfer function and the bits stay."""
        self._check(self._L.vr_hip_set_second_volume(self._ctx, None, 0, 0, 0, 0), "clear_second_volume")

    def set_second_transfer_fn(self, tf_premult, fused_esl):
        """vr_hip_set_second_transfer_fn: field B's premultiplied (128, 4) transfer function and the fused frame's 1024 leaping words —
        fused_esl(bits of A under A's function, bits of B under B's function).  Both are required."""
        tf = np.ascontiguousarray(tf_premult, dtype=np.float32)
        esl = np.ascontiguousarray(fused_esl, dtype=np.uint32)
        if tf.size != 512 or esl.size != 1024:
            raise VrError(1, "transfer_fn must be 128x4 floats and fused_esl 1024 words")
        self._check(self._L.vr_hip_set_second_transfer_fn(self._ctx, tf.ctypes.data, esl.ctypes.data), "set_second_transfer_fn")

    def render_fused(self, params, weight_a=1.0, weight_b=1.0, mode="sum"):
        """Host-buffer flavour: the composite frame over both fields; an (out_rows, out_width, 4) uint8 array.  mode "sum" adds the weighted
        colours of a sample before one accumulation, "over" accumulates field A's in front of field B's.  The context's clip, lighting and
        shadow apply to field A; field B is emissive.  params.sampling must be one of the TRILINEAR modes."""
        return self._host_frame("render_fused", "vr_hip_render_fused", params, C.byref(make_fusion(weight_a, weight_b, mode)), composite=True)

    def render_fused_device(self, params, dev_ptr, stream=None, weight_a=1.0, weight_b=1.0, mode="sum"):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None)."""
        self._frame("render_fused_device", "vr_hip_render_fused_device", params, C.byref(make_fusion(weight_a, weight_b, mode)), C.c_void_p(dev_ptr),
                    _ptr(stream), composite=True)

    def fused_frames(self):
        """vr_hip_fused_frames: the fused frames this context launched"""
        return self._counter("fused_frames", self._L.vr_hip_fused_frames)
