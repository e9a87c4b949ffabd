"""HipRenderer — python face of the C ABI context (include/vr_hip.h); method names follow the reference's Renderer
interface (VolumeRendering/Renderer.h:13-28)."""
import ctypes as C

import numpy as np

from .binding import (VrBackdrop, VrDepthOut, VrError, VrIso, VrLabelEntry, VrLaunchInfo, VrPick, VrRunAlignedInfo, VrTiming, VrVolumeInfo, lib, make_clip, make_depth,
                      make_label_entry, make_lighting, make_section, make_shadow)


def _rgba(params):
    """the (out_rows, out_width, 4) uint8 array a host-buffer frame fills"""
    return np.empty((params.out_rows, params.out_width, 4), dtype=np.uint8)


def _floats(params, wanted=True):
    """the (out_rows, out_width) float32 array of an optional host buffer (depth, value, alpha), None when it is not wanted"""
    return np.empty((params.out_rows, params.out_width), dtype=np.float32) if wanted else None


def _address(array):
    return array.ctypes.data if array is not None else None


def _ptr(address):
    """an optional device address or raw hipStream_t as the ABI takes it: NULL for None / 0"""
    return C.c_void_p(address) if address else None


class _Frames:
    """What HipRenderer and MultiRenderer share: the one call every frame goes through, and the shadow whose march step waits for a frame.
    The class names its handle (_handle) and its shadow setter (_SET_SHADOW) and brings _L and _check."""

    def _frame(self, what, entry, params, *args, composite):
        """One frame: `entry`(handle, params, *args).  A composite-type frame (the composite itself and everything that runs a composite
        pass: backdrop, hybrid, section in volume, labelled) first resolves a pending set_shadow(step=None); every other frame does not."""
        if composite:
            self._resolve_shadow(params.ray_step)
        self._check(getattr(self._L, entry)(self._handle, C.byref(params), *args), what)

    def _host_frame(self, what, entry, params, *args, composite, depth=None):
        """A host-buffer frame: `entry`(handle, params, *args, rgba[, depth]) into fresh arrays -> rgba, or (rgba, depth) for depth=True;
        depth=None: the entry takes no depth buffer."""
        out, dep = _rgba(params), _floats(params, bool(depth))
        self._frame(what, entry, params, *args, out.ctypes.data, *(() if depth is None else (_address(dep),)), composite=composite)
        return (out, dep) if depth else out

    def _set_shadow(self, shadow, what):
        self._check(getattr(self._L, self._SET_SHADOW)(self._handle, C.byref(shadow) if shadow is not None else None), what)

    def _hold_shadow(self, light_pos, dims, step, strength, cutoff, sampling):
        """set_shadow of both classes: step=None keeps the arguments in _shadow until a frame's ray_step resolves the step"""
        pending = None
        if step is None:
            pending = dict(light_pos=tuple(float(v) for v in light_pos), dims=dims, strength=strength, cutoff=cutoff, sampling=sampling)
            step = 0.01                  # validated now with a placeholder, set again with the frame's ray_step (an identical struct rebuilds nothing)
        self._set_shadow(make_shadow(light_pos, dims, step, strength, cutoff, sampling), "set_shadow")
        self._shadow = pending           # (a refused shadow leaves the one before in place)

    def clear_shadow(self):
        """Shadows off (the default)."""
        self._shadow = None
        self._set_shadow(None, "clear_shadow")

    def _resolve_shadow(self, ray_step):
        """a set_shadow(step=None) takes this step, once"""
        if self._shadow is not None:
            self._set_shadow(make_shadow(step=float(ray_step), **self._shadow), "set_shadow")
            self._shadow = None


class HipRenderer(_Frames):
    _SET_SHADOW = "vr_hip_set_shadow"
    _handle = property(lambda self: self._ctx)

    def __init__(self, device=0):
        self._L = lib()
        self._ctx = C.c_void_p()
        rc = self._L.vr_hip_create(int(device), C.byref(self._ctx))
        if rc:
            msg = self._L.vr_hip_last_error(self._ctx).decode() if self._ctx else "no usable HIP device; there is no CPU fallback"
            if self._ctx:
                self._L.vr_hip_destroy(self._ctx)
                self._ctx = C.c_void_p()
            raise VrError(rc, msg)
        self.device = int(device)
        self.dims = None
        self.bytes_per_voxel = None
        self._shadow = None              # set_shadow(step=None): the arguments, until a frame's ray_step resolves the step

    # -- lifetime
    def close(self):
        if self._ctx:
            self._L.vr_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise VrError(rc, f"{what}: {self._L.vr_hip_last_error(self._ctx).decode()}")

    def _counter(self, what, entry):
        """one of the testing aids that count the frames a family of kernels launched"""
        n = C.c_uint64(0)
        self._check(entry(self._ctx, C.byref(n)), what)
        return int(n.value)

    def get_name(self):
        return "HIP MI355X"

    # -- Renderer::set_*
    def set_window_buffer(self, width, height):
        self._check(self._L.vr_hip_set_window(self._ctx, width, height), "set_window_buffer")

    def set_transfer_fn(self, tf_premult, esl_bits):
        tf = np.ascontiguousarray(tf_premult, dtype=np.float32)
        esl = np.ascontiguousarray(esl_bits, dtype=np.uint32)
        if tf.size != 512 or esl.size != 1024:
            raise VrError(1, "transfer_fn must be 128x4 floats and esl 1024 words")
        self._check(self._L.vr_hip_set_transfer_fn(self._ctx, tf.ctypes.data, esl.ctypes.data), "set_transfer_fn")

    def set_volume(self, voxels):
        """voxels: numpy array shaped (z, y, x), uint8 or uint16."""
        v = np.ascontiguousarray(voxels)
        if v.dtype not in (np.uint8, np.uint16) or v.ndim != 3:
            raise VrError(1, "volume must be a 3-D uint8 / uint16 array")
        z, y, x = v.shape
        self._check(self._L.vr_hip_set_volume(self._ctx, v.ctypes.data, x, y, z, v.dtype.itemsize), "set_volume")
        self.dims, self.bytes_per_voxel = (x, y, z), v.dtype.itemsize

    def set_volume_device(self, dev_ptr, dims, bytes_per_voxel):
        self._check(self._L.vr_hip_set_volume_device(self._ctx, C.c_void_p(dev_ptr), dims[0], dims[1], dims[2], bytes_per_voxel),
                    "set_volume_device")
        self.dims, self.bytes_per_voxel = tuple(dims), bytes_per_voxel

    def set_layout(self, layout):
        """LAYOUT_LINEAR | LAYOUT_BRICKED for the TRILINEAR copy of the volume (images are identical, speed is not)."""
        self._check(self._L.vr_hip_set_layout(self._ctx, int(layout)), "set_layout")

    def set_wide_addressing(self, force):
        """Testing aid: 1 = arithmetic 64-bit path, 2 = 64-bit table path (what volumes > 1024^3 use), 0/False = automatic."""
        self._check(self._L.vr_hip_set_wide_addressing(self._ctx, int(force)), "set_wide_addressing")

    def set_brick_plane(self, plane=-1):
        """Brick copy for the TRILINEAR fetch: -1 per view (default), 0 / 1 / 2 = chunk plane (x,y) / (x,z) / (y,z); speed only."""
        self._check(self._L.vr_hip_set_brick_plane(self._ctx, int(plane)), "set_brick_plane")

    def set_column_copy(self, mode=0):
        """TRILINEAR column march: 0 voxel windows where a wave's columns fit, lit frames shading from the quad-element windows (default),
        1 quad-element windows, 2 voxel windows only (no second copy); speed and memory only."""
        self._check(self._L.vr_hip_set_column_copy(self._ctx, int(mode)), "set_column_copy")

    def set_run_flavour(self, flavour=0):
        """Run bricks of full-march frames: 0 automatic (default), 1 nine-element runs, 2 seven-cell aligned runs; speed and memory only."""
        self._check(self._L.vr_hip_set_run_flavour(self._ctx, int(flavour)), "set_run_flavour")

    def run_aligned_info(self):
        """vr_run_aligned_info: dict(flavour, last_flavour (0 no run bricks, 1 nine-element, 2 aligned), copies, copies_refused, bytes, build_ms (z, y))."""
        info = VrRunAlignedInfo()
        self._check(self._L.vr_hip_run_aligned_info(self._ctx, C.byref(info)), "run_aligned_info")
        return {"flavour": int(info.flavour), "last_flavour": int(info.last_flavour), "copies": int(info.copies), "copies_refused": int(info.copies_refused),
                "bytes": int(info.bytes), "build_ms": (float(info.build_ms[0]), float(info.build_ms[1]))}

    def set_tile_mapping(self, lane_map=-1, phase_x=0, phase_y=0):
        """Lane order inside a 4x4-pixel block (-1 automatic, 0 rows, 1 columns, 2 2x2 blocks) and tile-grid phase; speed only."""
        self._check(self._L.vr_hip_set_tile_mapping(self._ctx, int(lane_map), int(phase_x), int(phase_y)), "set_tile_mapping")

    def set_tile_scheduling(self, mode=1):
        """0: tile = workgroup id; 1 (default): measured-cost order for frames with ESL / ERT on (most expensive tiles first); speed only."""
        self._check(self._L.vr_hip_set_tile_scheduling(self._ctx, int(mode)), "set_tile_scheduling")

    def set_clip(self, box_min=None, box_max=None, plane=None):
        """vr_hip_set_clip: every later composite, MIP and isosurface frame is cropped to the box [box_min, box_max] (model space: the cube
        is [-1,1]^3; missing = the whole cube) and cut by the plane (nx, ny, nz, d), keeping nx*x + ny*y + nz*z + d >= 0 (missing = none)."""
        self._check(self._L.vr_hip_set_clip(self._ctx, C.byref(make_clip(box_min, box_max, plane))), "set_clip")

    def clear_clip(self):
        """Clipping off (the default)."""
        self._check(self._L.vr_hip_set_clip(self._ctx, None), "clear_clip")

    def set_shadow(self, light_pos, dims=128, step=None, strength=1.0, cutoff=1.0 / 256.0, sampling=1):
        """vr_hip_set_shadow: every later COMPOSITE frame darkens its dense samples by what lies between them and the light at `light_pos`
        (model space: the cube is [-1,1]^3).  dims = nodes per edge of the light grid (2..256); step = the march step towards the light, None =
        the ray_step of the NEXT composite frame (resolved once, at that frame: shadows as dense as it sees them; later frames with another
        ray_step keep that step — call set_shadow again to follow them; until then download_shadow needs its ray_step argument); strength 0..1 (0 = unshadowed bytes);
        cutoff = the transmittance below which a light ray is black; sampling = how the builder samples the volume.  The frames must be
        TRILINEAR / TRILINEAR_Q8; MIP and isosurface frames ignore the shadow.  The light of the frames' own shading is params.view.light_pos:
        set it to the same point for a consistent picture."""
        self._hold_shadow(light_pos, dims, step, strength, cutoff, sampling)

    def download_shadow(self, ray_step=None):
        """vr_hip_download_shadow: the light grid as a (S, S, S) uint8 array indexed [z, y, x], 255 = fully lit; builds it if stale.  After a
        set_shadow(step=None) that no frame has resolved yet, ray_step is required and resolves it the way a frame with that ray_step would."""
        if self._shadow is not None:
            if ray_step is None:
                raise VrError(1, "download_shadow: set_shadow(step=None) has no step yet — render a frame first or pass ray_step")
            self._resolve_shadow(ray_step)
        dims = C.c_uint32(0)
        self._check(self._L.vr_hip_download_shadow(self._ctx, None, 0, C.byref(dims)), "download_shadow")       # size query
        out = np.empty((dims.value,) * 3, dtype=np.uint8)
        self._check(self._L.vr_hip_download_shadow(self._ctx, out.ctypes.data, out.nbytes, C.byref(dims)), "download_shadow")
        return out

    def shadow_builds(self):
        """(number of light-grid builds of this context, hipEvent ms of the last one)"""
        n, ms = C.c_uint64(0), C.c_float(0)
        self._check(self._L.vr_hip_shadow_builds(self._ctx, C.byref(n), C.byref(ms)), "shadow_builds")
        return int(n.value), float(ms.value)

    def set_lighting(self, ambient=0.25, diffuse=0.65, specular=0.4, shininess_log2=4):
        """vr_hip_set_lighting: every later COMPOSITE frame shades its dense samples from the gradient of the interpolated field — ambient +
        diffuse * |n.l| (two-sided) on the looked-up colour and a white highlight specular * |n.h|^(2^shininess_log2) — in place of the
        reference's cue; params.light_kd is then ignored and the light is params.view.light_pos.  Coefficients 0..1, shininess_log2 0..10.
        The frames must be TRILINEAR / TRILINEAR_Q8; MIP and isosurface frames ignore the lighting; a shadow and a clip compose with it."""
        self._check(self._L.vr_hip_set_lighting(self._ctx, C.byref(make_lighting(ambient, diffuse, specular, shininess_log2))), "set_lighting")

    def clear_lighting(self):
        """Gradient lighting off (the default): the reference's cue again."""
        self._check(self._L.vr_hip_set_lighting(self._ctx, None), "clear_lighting")

    def lighting_frames(self):
        """vr_hip_lighting_frames: the composite frames this context launched on the gradient-lit kernels"""
        return self._counter("lighting_frames", self._L.vr_hip_lighting_frames)

    def set_preintegration(self, on=True):
        """vr_hip_set_preintegration: every later COMPOSITE frame classifies the slab between two consecutive samples — the mean of the
        piecewise-linear transfer function between the previous sample's value and its own, from the integral table K — in place of one
        lookup per sample.  The frames must be TRILINEAR / TRILINEAR_Q8; MIP and isosurface frames ignore it; clip, shadow and lighting
        compose with it.  `on` is passed through as an integer: anything but 0 / 1 / False / True is VR_ERR_INVALID."""
        self._check(self._L.vr_hip_set_preintegration(self._ctx, int(on)), "set_preintegration")

    def clear_preintegration(self):
        """Pre-integration off (the default): one transfer-function lookup per sample again."""
        self._check(self._L.vr_hip_set_preintegration(self._ctx, 0), "clear_preintegration")

    def preint_frames(self):
        """vr_hip_preint_frames: the composite frames this context launched on the slab kernels"""
        return self._counter("preint_frames", self._L.vr_hip_preint_frames)

    def download_tf_integral(self):
        """vr_hip_download_tf_integral: K as uploaded, [128, 4] float32"""
        out = np.zeros((128, 4), np.float32)
        self._check(self._L.vr_hip_download_tf_integral(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), "download_tf_integral")
        return out

    def last_launch(self):
        """What the last render launched: dict(layout, brick_plane, lane_map, phase_x, phase_y, clamp_fetch, tiles_x, tiles_y, ordered, straddle_permille,
        column_voxels, column_shade_pairs, shadowed) and, from vr_hip_run_aligned_info, run_flavour (0 no run bricks, 1 nine-element runs, 2 aligned runs)."""
        info = VrLaunchInfo()
        self._check(self._L.vr_hip_last_launch(self._ctx, C.byref(info)), "last_launch")
        out = {n: int(getattr(info, n)) for n, _ in VrLaunchInfo._fields_}
        out["run_flavour"] = self.run_aligned_info()["last_flavour"]
        return out

    def tile_costs(self):
        """Cost map of the last frame rendered with set_tile_scheduling(2): [tiles_y, tiles_x] uint32, 64-cycle units per workgroup tile."""
        tx, ty = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.vr_hip_read_tile_costs(self._ctx, None, 0, C.byref(tx), C.byref(ty)), "read_tile_costs")
        out = np.zeros((ty.value, tx.value), dtype=np.uint32)
        self._check(self._L.vr_hip_read_tile_costs(self._ctx, out.ctypes.data, out.size, C.byref(tx), C.byref(ty)), "read_tile_costs")
        return out

    def generate_volume(self, kind, n, seed=1, bytes_per_voxel=1):
        """Synthetic benchmark volume ('shell' | 'noise') generated straight into HBM."""
        k = {"shell": 0, "noise": 1}[kind]
        self._check(self._L.vr_hip_generate_volume(self._ctx, k, n, seed, bytes_per_voxel), "generate_volume")
        self.dims, self.bytes_per_voxel = (n, n, n), bytes_per_voxel

    def download_volume(self):
        x, y, z = self.dims
        out = np.empty((z, y, x), dtype=np.uint8 if self.bytes_per_voxel == 1 else np.uint16)
        self._check(self._L.vr_hip_download_volume(self._ctx, out.ctypes.data, out.nbytes), "download_volume")
        return out

    # -- Renderer::render_volume
    def render_volume(self, params):
        """Host-buffer flavour (reference renderer ids 0-2): returns an (out_rows, out_width, 4) uint8 array."""
        return self._host_frame("render_volume", "vr_hip_render", params, composite=True)

    def render_volume_device(self, params, dev_ptr, stream=None):
        """Device-buffer flavour (ids 3-4): asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None)."""
        self._frame("render_volume_device", "vr_hip_render_device", params, C.c_void_p(dev_ptr), _ptr(stream), composite=True)

    # -- maximum-intensity projection (vr_hip_render_mip: the maximum sample of every ray through one transfer-function lookup)
    def render_mip(self, params):
        """Host-buffer flavour: returns an (out_rows, out_width, 4) uint8 array.  params.esl != 0 = exact fetch skipping by block maxima."""
        return self._host_frame("render_mip", "vr_hip_render_mip", params, composite=False)

    def render_mip_device(self, params, dev_ptr, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None)."""
        self._frame("render_mip_device", "vr_hip_render_mip_device", params, C.c_void_p(dev_ptr), _ptr(stream), composite=False)

    # -- shaded isosurface with depth (vr_hip_render_iso: the first sample along every ray that reaches `level`, refined by bisection)
    def render_iso(self, params, level, refine=4, depth=False):
        """Host-buffer flavour: an (out_rows, out_width, 4) uint8 array, or with depth=True (rgba, depth): depth is float32
        (out_rows, out_width), the ray parameter k of the surface point (position = origin + direction * k of the pixel's own ray; the
        perspective direction is not normalised) and -1 where there is none.  `level` in raw voxel units; params.sampling must be one of
        the TRILINEAR modes; params.esl != 0 = exact fetch skipping by block maxima."""
        return self._host_frame("render_iso", "vr_hip_render_iso", params, C.byref(VrIso(float(level), int(refine))), composite=False, depth=bool(depth))

    def render_iso_device(self, params, level, refine, dev_ptr, depth_ptr=None, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` (RGBA8) and, if given, `depth_ptr` (float32) on `stream` (raw hipStream_t or None)."""
        self._frame("render_iso_device", "vr_hip_render_iso_device", params, C.byref(VrIso(float(level), int(refine))), C.c_void_p(dev_ptr), _ptr(depth_ptr), _ptr(stream),
                    composite=False)

    # -- backdrop and hybrid (vr_hip_render_backdrop / vr_hip_render_hybrid: a composite frame that stops at an opaque layer and blends over it)
    def render_backdrop(self, params, rgba, depth):
        """Host-buffer flavour: the composite frame (with the context's clip, shadow, lighting and pre-integration) over the opaque layer
        `rgba` ((out_rows, out_width, 4) uint8, premultiplied) at `depth` ((out_rows, out_width) float32: k of the pixel's own ray, the
        isosurface frame's depth; negative or NaN = no surface, +inf = behind everything).  Returns an (out_rows, out_width, 4) uint8 array.
        params.sampling must be one of the TRILINEAR modes."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if rgba.size != params.out_rows * params.out_width * 4 or depth.size != params.out_rows * params.out_width:
            raise ValueError("render_backdrop: the layers must have out_rows * out_width pixels")
        return self._host_frame("render_backdrop", "vr_hip_render_backdrop", params, C.byref(VrBackdrop(rgba.ctypes.data, depth.ctypes.data)), composite=True)

    def render_backdrop_device(self, params, rgba_ptr, depth_ptr, dev_ptr, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None); the layers are device addresses,
        and `dev_ptr` may be `rgba_ptr` (in place)."""
        self._frame("render_backdrop_device", "vr_hip_render_backdrop_device", params, C.byref(VrBackdrop(rgba_ptr or None, depth_ptr or None)), C.c_void_p(dev_ptr), _ptr(stream),
                    composite=True)

    def render_hybrid(self, params, level, refine=4, depth=False):
        """Host-buffer flavour of the hybrid: the isosurface of `level` (render_iso with the same arguments) seen through the translucent
        volume in front of it.  An (out_rows, out_width, 4) uint8 array, or with depth=True (rgba, depth): the isosurface's depth."""
        return self._host_frame("render_hybrid", "vr_hip_render_hybrid", params, C.byref(VrIso(float(level), int(refine))), composite=True, depth=bool(depth))

    def render_hybrid_device(self, params, level, refine, dev_ptr, depth_ptr=None, stream=None):
        """Device-buffer flavour: the isosurface frame into `dev_ptr` and `depth_ptr` (a context-owned buffer when None), then the backdrop
        frame in place, both on `stream` (raw hipStream_t or None)."""
        self._frame("render_hybrid_device", "vr_hip_render_hybrid_device", params, C.byref(VrIso(float(level), int(refine))), C.c_void_p(dev_ptr), _ptr(depth_ptr), _ptr(stream),
                    composite=True)

    def backdrop_frames(self):
        """vr_hip_backdrop_frames: the composite frames this context launched on the backdrop kernels"""
        return self._counter("backdrop_frames", self._L.vr_hip_backdrop_frames)

    # -- section frames (vr_hip_render_section: the oblique slice through the interpolated field, its thick-slab MIP / MinIP / mean, with depth)
    def render_section(self, params, plane, half_width=0.0, mode="point", window=None, depth=False):
        """Host-buffer flavour: the section n.x*x + n.y*y + n.z*z + d = 0 (`plane` = (n.x, n.y, n.z, d), model space) as an
        (out_rows, out_width, 4) uint8 array, or with depth=True (rgba, depth): depth is float32 (out_rows, out_width), k of the section
        point (thick modes: of the slab's front face) on the pixel's own ray, -1 where there is none.  mode "point", or with half_width > 0
        "max", "min", "mean" over the slab; window (lo, hi) in raw voxel units = opaque grey, None = the transfer function.
        params.sampling must be one of the TRILINEAR modes."""
        return self._host_frame("render_section", "vr_hip_render_section", params, C.byref(make_section(plane, half_width, mode, window)), composite=False, depth=bool(depth))

    def render_section_device(self, params, plane, half_width, mode, window, dev_ptr, depth_ptr=None, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` (RGBA8) and, if given, `depth_ptr` (float32) on `stream` (raw hipStream_t or None)."""
        self._frame("render_section_device", "vr_hip_render_section_device", params, C.byref(make_section(plane, half_width, mode, window)), C.c_void_p(dev_ptr), _ptr(depth_ptr),
                    _ptr(stream), composite=False)

    def render_section_in_volume(self, params, plane, half_width=0.0, mode="point", window=None, depth=False):
        """Host-buffer flavour of the section inside the volume: render_section with the same arguments seen through the translucent volume
        in front of it (the context's clip, shadow, lighting and pre-integration apply to the composite pass).  An (out_rows, out_width, 4)
        uint8 array, or with depth=True (rgba, depth): the section's depth."""
        return self._host_frame("render_section_in_volume", "vr_hip_render_section_in_volume", params, C.byref(make_section(plane, half_width, mode, window)), composite=True,
                                depth=bool(depth))

    def render_section_in_volume_device(self, params, plane, half_width, mode, window, dev_ptr, depth_ptr=None, stream=None):
        """Device-buffer flavour: the section frame into `dev_ptr` and `depth_ptr` (a context-owned buffer when None), then the backdrop frame
        in place, both on `stream` (raw hipStream_t or None)."""
        self._frame("render_section_in_volume_device", "vr_hip_render_section_in_volume_device", params, C.byref(make_section(plane, half_width, mode, window)), C.c_void_p(dev_ptr),
                    _ptr(depth_ptr), _ptr(stream), composite=True)

    def section_frames(self):
        """vr_hip_section_frames: the section frames this context launched"""
        return self._counter("section_frames", self._L.vr_hip_section_frames)

    # -- depth frames of the composite and picking (vr_hip_render_depth, vr_hip_pick)
    def render_depth(self, params, opacity, mode="first", value=False, alpha=False):
        """Host-buffer flavour: where along its ray the thing a composite pixel shows lies, float32 (out_rows, out_width): k of the pixel's own
        ray, -1 where there is no surface.  mode "first" (the first sample at which the accumulated alpha reaches `opacity`), "peak" (the
        sample that contributes most) or "mean" (the contribution-weighted mean).  value=True adds the interpolated raw value there, alpha=True
        the pixel's final alpha — the alpha channel of the composite frame before it becomes a byte: (depth[, value][, alpha]).  The
        context's clip and pre-integration apply; shadow and lighting are ignored.  params.sampling must be one of the TRILINEAR modes."""
        dep, val, alp = _floats(params), _floats(params, value), _floats(params, alpha)
        out = VrDepthOut(dep.ctypes.data, _address(val), _address(alp))
        self._frame("render_depth", "vr_hip_render_depth", params, C.byref(make_depth(opacity, mode)), C.byref(out), composite=False)
        got = tuple(a for a in (dep, val, alp) if a is not None)
        return got if len(got) > 1 else dep

    def render_depth_device(self, params, opacity, mode, depth_ptr, value_ptr=None, alpha_ptr=None, stream=None):
        """Device-buffer flavour: asynchronous launch into `depth_ptr` and, if given, `value_ptr` and `alpha_ptr` (float32 each) on `stream`
        (raw hipStream_t or None)."""
        out = VrDepthOut(depth_ptr or None, value_ptr or None, alpha_ptr or None)
        self._frame("render_depth_device", "vr_hip_render_depth_device", params, C.byref(make_depth(opacity, mode)), C.byref(out), _ptr(stream), composite=False)

    def pick(self, params, pixels, opacity, mode="first"):
        """What a whole-frame depth frame of `params` stores at each of `pixels` ((x, y) pairs of the view, y up; at most 256), as a list of
        dicts: hit, k, position (model space), voxel (continuous voxel index), value, alpha.  The partition fields of params are ignored."""
        d = make_depth(opacity, mode)
        xy = np.ascontiguousarray(np.asarray(pixels, dtype=np.int64).reshape(-1, 2))
        n = xy.shape[0]
        if (xy < 0).any() or (xy > 0xffffffff).any():
            raise VrError(1, "pick: a pixel lies outside the window")
        xy = xy.astype(np.uint32)
        out = (VrPick * max(n, 1))()
        self._check(self._L.vr_hip_pick(self._ctx, C.byref(params), C.byref(d), n, xy.ctypes.data_as(C.POINTER(C.c_uint32)), out), "pick")
        return [{"hit": bool(o.hit), "k": float(o.k), "position": tuple(o.position), "voxel": tuple(o.voxel), "value": float(o.value), "alpha": float(o.alpha)}
                for o in out[:n]]

    def depth_frames(self):
        """vr_hip_depth_frames: the depth frames this context launched (a pick counts one per pixel)"""
        return self._counter("depth_frames", self._L.vr_hip_depth_frames)

    # -- label volumes (vr_hip_set_labels, vr_hip_set_label_table, vr_hip_render_labelled: per-segment colour and visibility for composite frames)
    def set_labels(self, labels):
        """vr_hip_set_labels: the segment of every voxel, one byte each, with the dims of the resident volume.  `labels` is a numpy array
        shaped (z, y, x) of uint8, or a contiguous uint8 device tensor of that shape (copied on the context's stream).  A new volume drops them."""
        if hasattr(labels, "data_ptr"):
            if str(labels.dtype) != "torch.uint8" or labels.dim() != 3 or not labels.is_contiguous() or not labels.is_cuda:
                raise VrError(1, "labels must be a contiguous 3-D uint8 device tensor")
            z, y, x = (int(n) for n in labels.shape)
            self._check(self._L.vr_hip_set_labels_device(self._ctx, C.c_void_p(labels.data_ptr()), x, y, z), "set_labels")
            return
        v = np.ascontiguousarray(labels)
        if v.dtype != np.uint8 or v.ndim != 3:
            raise VrError(1, "labels must be a 3-D uint8 array")
        z, y, x = v.shape
        self._check(self._L.vr_hip_set_labels(self._ctx, v.ctypes.data, x, y, z), "set_labels")

    def clear_labels(self):
        """Drops the labels: render_labelled is VR_ERR_NOT_READY until they are set again.  The table stays."""
        self._check(self._L.vr_hip_set_labels(self._ctx, None, 0, 0, 0), "clear_labels")

    def set_label_table(self, entries=None):
        """vr_hip_set_label_table: what each label does to a sample's classified colour.  `entries`: at most 256 of VrLabelEntry, dict(colour,
        mix, opacity) or (r, g, b, mix, opacity), entry i for label i; the rest — and everything for None — are the identity (mix 0, opacity 1)."""
        items = list(entries) if entries is not None else []
        table = (VrLabelEntry * max(len(items), 1))()
        for i, e in enumerate(items):
            if isinstance(e, VrLabelEntry):
                table[i] = e
            elif isinstance(e, dict):
                table[i] = make_label_entry(**e)
            else:
                table[i] = make_label_entry(e[0:3], e[3], e[4])
        self._check(self._L.vr_hip_set_label_table(self._ctx, table if items else None, len(items)), "set_label_table")

    def render_labelled(self, params):
        """Host-buffer flavour: the composite frame with every sample's colour passed through the table entry of its nearest voxel's label; an
        (out_rows, out_width, 4) uint8 array.  The context's clip, lighting and shadow apply; params.sampling must be one of the TRILINEAR modes."""
        return self._host_frame("render_labelled", "vr_hip_render_labelled", params, composite=True)

    def render_labelled_device(self, params, dev_ptr, stream=None):
        """Device-buffer flavour: asynchronous launch into `dev_ptr` on `stream` (raw hipStream_t or None)."""
        self._frame("render_labelled_device", "vr_hip_render_labelled_device", params, C.c_void_p(dev_ptr), _ptr(stream), composite=True)

    def labelled_frames(self):
        """vr_hip_labelled_frames: the labelled frames this context launched"""
        return self._counter("labelled_frames", self._L.vr_hip_labelled_frames)

    # -- timing (Profiler.cpp:46-67)
    def timing(self):
        t = VrTiming()
        self._check(self._L.vr_hip_timing(self._ctx, C.byref(t)), "timing")
        return t

    def timing_reset(self):
        self._check(self._L.vr_hip_timing_reset(self._ctx), "timing_reset")

    # -- feeders on the GPU
    def volume_minmax(self):
        mm = np.empty((32 * 32 * 32, 2), dtype=np.uint8)
        bd = C.c_uint32()
        bs = (C.c_float * 3)()
        ms = C.c_float()
        self._check(self._L.vr_hip_volume_minmax(self._ctx, mm.ctypes.data, C.byref(bd), bs, C.byref(ms)), "volume_minmax")
        return mm, int(bd.value), tuple(float(v) for v in bs), float(ms.value)

    def volume_histogram(self):
        h = np.empty(256, dtype=np.uint64)
        ms = C.c_float()
        self._check(self._L.vr_hip_volume_histogram(self._ctx, h.ctypes.data, C.byref(ms)), "volume_histogram")
        return h, float(ms.value)

    def volume_info(self):
        """vr_volume_info: what the resident volume occupies (how many brick copies were actually built, linear array present)."""
        info = VrVolumeInfo()
        self._check(self._L.vr_hip_volume_info(self._ctx, C.byref(info)), "volume_info")
        return info

    def prepare(self, copies=8191):
        """vr_hip_prepare: build the brick copies named by the VR_COPY_* bits now instead of on first use (default: all the
        layout policy has at this size).  A refused copy (HBM guard) raises VrError(VR_ERR_ALLOC); frames then read the next best."""
        self._check(self._L.vr_hip_prepare(self._ctx, int(copies)), "prepare")

    def download_copy(self, kind):
        """vr_hip_download_copy (testing aid): the raw bytes of resident brick copy `kind` (bit index of its VR_COPY_* flag)."""
        n = C.c_uint64()
        self._check(self._L.vr_hip_download_copy(self._ctx, int(kind), None, 0, C.byref(n)), "download_copy")
        out = np.empty(n.value, dtype=np.uint8)
        self._check(self._L.vr_hip_download_copy(self._ctx, int(kind), out.ctypes.data, out.nbytes, None), "download_copy")
        return out

    def release_linear_copy(self):
        """Frees the linear array (feeders / download / layout changes then need a new set_volume); rendering is unaffected."""
        self._check(self._L.vr_hip_release_linear_copy(self._ctx), "release_linear_copy")

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_uint32()
        mem = C.c_uint64()
        self._check(self._L.vr_hip_device_info(self._ctx, name, 256, C.byref(cus), C.byref(mem)), "device_info")
        return name.value.decode(), int(cus.value), int(mem.value)


class MultiRenderer(_Frames):
    """Several GPUs of ONE process behind one render call (vr_hip_multi_* of include/vr_hip.h): interleaved bands per device,
    gathered on devices[0] over xGMI (RCCL send/recv, or peer copies), de-interleaved there.  `params` describe the whole frame."""
    _SET_SHADOW = "vr_hip_multi_set_shadow"
    _handle = property(lambda self: self._m)

    def __init__(self, devices):
        self._L = lib()
        self._m = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = self._L.vr_hip_multi_create(len(devices), devs, C.byref(self._m))
        if rc:
            msg = self._L.vr_hip_multi_last_error(self._m).decode() if self._m else "no usable HIP device; there is no CPU fallback"
            if self._m:
                self._L.vr_hip_multi_destroy(self._m)
                self._m = C.c_void_p()
            raise VrError(rc, msg)
        self.devices = list(devices)
        self._shadow = None

    def close(self):
        if self._m:
            self._L.vr_hip_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise VrError(rc, f"{what}: {self._L.vr_hip_multi_last_error(self._m).decode()}")

    @property
    def transport(self):
        return self._L.vr_hip_multi_transport(self._m).decode()

    def set_window_buffer(self, width, height):
        self._check(self._L.vr_hip_multi_set_window(self._m, width, height), "set_window_buffer")

    def set_transfer_fn(self, tf_premult, esl_bits):
        tf = np.ascontiguousarray(tf_premult, dtype=np.float32)
        esl = np.ascontiguousarray(esl_bits, dtype=np.uint32)
        self._check(self._L.vr_hip_multi_set_transfer_fn(self._m, tf.ctypes.data, esl.ctypes.data), "set_transfer_fn")

    def set_clip(self, box_min=None, box_max=None, plane=None):
        """vr_hip_multi_set_clip: HipRenderer.set_clip on every device's context."""
        self._check(self._L.vr_hip_multi_set_clip(self._m, C.byref(make_clip(box_min, box_max, plane))), "set_clip")

    def clear_clip(self):
        self._check(self._L.vr_hip_multi_set_clip(self._m, None), "clear_clip")

    def set_shadow(self, light_pos, dims=128, step=None, strength=1.0, cutoff=1.0 / 256.0, sampling=1):
        """vr_hip_multi_set_shadow: HipRenderer.set_shadow on every device's context (every device builds its own light grid); step=None
        is resolved once, by the next frame's ray_step."""
        self._hold_shadow(light_pos, dims, step, strength, cutoff, sampling)

    def set_lighting(self, ambient=0.25, diffuse=0.65, specular=0.4, shininess_log2=4):
        """vr_hip_multi_set_lighting: HipRenderer.set_lighting on every device's context"""
        self._check(self._L.vr_hip_multi_set_lighting(self._m, C.byref(make_lighting(ambient, diffuse, specular, shininess_log2))), "set_lighting")

    def clear_lighting(self):
        self._check(self._L.vr_hip_multi_set_lighting(self._m, None), "clear_lighting")

    def set_preintegration(self, on=True):
        """vr_hip_multi_set_preintegration: HipRenderer.set_preintegration on every device's context"""
        self._check(self._L.vr_hip_multi_set_preintegration(self._m, int(on)), "set_preintegration")

    def set_volume(self, voxels):
        v = np.ascontiguousarray(voxels)
        z, y, x = v.shape
        self._check(self._L.vr_hip_multi_set_volume(self._m, v.ctypes.data, x, y, z, v.dtype.itemsize), "set_volume")

    def generate_volume(self, kind, n, seed=1, bytes_per_voxel=1):
        self._check(self._L.vr_hip_multi_generate_volume(self._m, {"shell": 0, "noise": 1}[kind], n, seed, bytes_per_voxel), "generate_volume")

    def render_volume(self, params):
        out = np.empty((params.view.height, params.view.width, 4), dtype=np.uint8)
        self._frame("render_volume", "vr_hip_multi_render", params, out.ctypes.data, composite=True)
        return out

    def render_volume_device(self, params, dev_ptr):
        self._frame("render_volume_device", "vr_hip_multi_render_device", params, C.c_void_p(dev_ptr), composite=True)

    def render_volume_device_async(self, params, dev_ptr, consumer_stream=None):
        """Queues a frame (up to THREE in flight: kFrames in vr_multi.cpp; frames in flight must not share `dev_ptr`); `consumer_stream`
        (raw hipStream_t on devices[0]) waits for the assembled frame."""
        self._frame("render_volume_device_async", "vr_hip_multi_render_device_async", params, C.c_void_p(dev_ptr), _ptr(consumer_stream), composite=True)

    def sync(self):
        self._check(self._L.vr_hip_multi_sync(self._m), "sync")

    def prepare(self, copies=8191):
        self._check(self._L.vr_hip_multi_prepare(self._m, int(copies)), "prepare")

    def context_timing(self, rank):
        """vr_timing of one device's context (kernel_ms_sum / launches since its last reset)."""
        t = VrTiming()
        rc = self._L.vr_hip_timing(C.c_void_p(self._L.vr_hip_multi_context(self._m, rank)), C.byref(t))
        if rc:
            raise VrError(rc, "vr_hip_timing")
        return t

    def timing(self):
        per = (C.c_float * len(self.devices))()
        total = C.c_float()
        self._check(self._L.vr_hip_multi_timing(self._m, per, C.byref(total)), "timing")
        return [float(x) for x in per], float(total.value)
