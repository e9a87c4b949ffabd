"""ctypes declarations of the C ABI in include/vr_hip.h and include/vr_host.h (struct layouts must match)."""
import ctypes as C
import os

SAMPLE_NEAREST = 0      # vr_sampling.VR_SAMPLE_NEAREST   — CPURenderer / GPURenderer1-3 semantics
SAMPLE_TRILINEAR = 1    # vr_sampling.VR_SAMPLE_TRILINEAR — GPURenderer4 semantics, fp32 filter weights
SAMPLE_TRILINEAR_Q8 = 2  # vr_sampling.VR_SAMPLE_TRILINEAR_Q8 — the same with 8-bit filter weights (the texture unit's definition)
LAYOUT_LINEAR = 0        # vr_layout
LAYOUT_BRICKED = 1
# VR_COPY_* bits (vr_hip_prepare / vr_volume_info.copies): quad bricks per chunk plane, run bricks along z / y, voxel bricks
COPY_QUAD_XY, COPY_QUAD_XZ, COPY_QUAD_YZ, COPY_RUN_Z, COPY_RUN_Y, COPY_VOXEL, COPY_OCT, COPY_COL_X, COPY_COL_Y, COPY_COL_Z, COPY_ALL = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 8191
COPY_COLV_X, COPY_COLV_Y, COPY_COLV_Z = 1024, 2048, 4096
# aligned run bricks along z / y (32-byte runs of seven cells): behind the COPY_KINDS kinds, not part of COPY_ALL; download_copy kinds 13 / 14
COPY_RUN7_Z, COPY_RUN7_Y = 1 << 13, 1 << 14
RUN_FLAVOUR_AUTO, RUN_FLAVOUR_NINE, RUN_FLAVOUR_SEVEN = 0, 1, 2      # vr_hip_set_run_flavour
COPY_NAMES = ("quad_xy", "quad_xz", "quad_yz", "run_z", "run_y", "voxel", "oct", "col_x", "col_y", "col_z", "colv_x", "colv_y", "colv_z")
COPY_KINDS = 13
TF_SIZE = 128
ESL_VOLUME_SIZE = 1024

_STATUS = {0: "VR_OK", 1: "VR_ERR_INVALID", 2: "VR_ERR_NO_DEVICE", 3: "VR_ERR_ALLOC", 4: "VR_ERR_HIP", 5: "VR_ERR_NOT_READY"}


class VrError(RuntimeError):
    def __init__(self, code, message=""):
        self.code = code
        super().__init__(f"{_STATUS.get(code, code)}: {message}" if message else _STATUS.get(code, str(code)))


class VrView(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("origin", C.c_float * 3), ("direction", C.c_float * 3), ("right_plane", C.c_float * 3),
        ("up_plane", C.c_float * 3), ("light_pos", C.c_float * 3), ("perspective", C.c_uint32),
    ]


class VrParams(C.Structure):
    _fields_ = [
        ("view", VrView),
        ("ray_step", C.c_float), ("ray_threshold", C.c_float), ("esl", C.c_uint32), ("esl_block_dims", C.c_uint32),
        ("esl_block_size", C.c_float * 3), ("light_kd", C.c_float), ("sampling", C.c_uint32),
        ("x0", C.c_uint32), ("out_width", C.c_uint32), ("out_rows", C.c_uint32),
        ("band_rows", C.c_uint32), ("band_stride", C.c_uint32), ("band_first", C.c_uint32),
    ]

    def copy(self):
        other = VrParams()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(VrParams))
        return other


class VrIso(C.Structure):
    """vr_iso: the level in RAW voxel units (0..255 / 0..65535) and the bisection steps after the first hit (0..16)"""
    _fields_ = [("level", C.c_float), ("refine", C.c_uint32)]


class VrClip(C.Structure):
    """vr_clip: the crop box in model space (the cube is [-1,1]^3) and the kept half-space n.x*x + n.y*y + n.z*z + d >= 0 (all four 0 = no plane)"""
    _fields_ = [("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("plane", C.c_float * 4)]


def make_clip(box_min=None, box_max=None, plane=None):
    """A VrClip; a missing box is [-1,1]^3, a missing plane is zeros (no plane)."""
    clip = VrClip()
    for i in range(3):
        clip.box_min[i] = -1.0 if box_min is None else float(box_min[i])
        clip.box_max[i] = 1.0 if box_max is None else float(box_max[i])
    for i in range(4):
        clip.plane[i] = 0.0 if plane is None else float(plane[i])
    return clip


class VrShadow(C.Structure):
    """vr_shadow: the light in model space, the nodes per edge of the light grid, the march step towards the light, strength 0..1, the
    transmittance below which a light ray is black, and how the builder samples the volume (SAMPLE_TRILINEAR / SAMPLE_TRILINEAR_Q8)"""
    _fields_ = [("light_pos", C.c_float * 3), ("dims", C.c_uint32), ("step", C.c_float), ("strength", C.c_float), ("cutoff", C.c_float),
                ("sampling", C.c_uint32)]


def make_shadow(light_pos, dims=128, step=0.01, strength=1.0, cutoff=1.0 / 256.0, sampling=SAMPLE_TRILINEAR):
    sh = VrShadow()
    for i in range(3):
        sh.light_pos[i] = float(light_pos[i])
    sh.dims, sh.step, sh.strength, sh.cutoff, sh.sampling = int(dims), float(step), float(strength), float(cutoff), int(sampling)
    return sh


class VrLighting(C.Structure):
    """vr_lighting: ambient, diffuse and specular coefficients (0..1) and shininess_log2 (0..10: the highlight is raised to the power 2^n)"""
    _fields_ = [("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float), ("shininess_log2", C.c_uint32)]


def make_lighting(ambient=0.25, diffuse=0.65, specular=0.4, shininess_log2=4):
    if int(shininess_log2) < 0:
        raise ValueError("shininess_log2 must be in 0..10")
    return VrLighting(float(ambient), float(diffuse), float(specular), int(shininess_log2))


class VrBackdrop(C.Structure):
    """vr_backdrop: the opaque layer of a backdrop frame — RGBA8 words (premultiplied) and float depths (k of the pixel's own ray; negative or
    NaN = no surface), both laid out like the frame's output buffer"""
    _fields_ = [("rgba", C.c_void_p), ("depth", C.c_void_p)]


SECTION_POINT, SECTION_MAX, SECTION_MIN, SECTION_MEAN = 0, 1, 2, 3
SECTION_MODES = {"point": SECTION_POINT, "max": SECTION_MAX, "min": SECTION_MIN, "mean": SECTION_MEAN}


class VrSection(C.Structure):
    """vr_section: the plane n.x*x + n.y*y + n.z*z + d = 0 in model space, the slab's half width (0 for POINT), the mode (SECTION_*) and the
    grey window lo, hi in RAW voxel units (both 0 = colour by the transfer function)"""
    _fields_ = [("plane", C.c_float * 4), ("half_width", C.c_float), ("mode", C.c_uint32), ("window", C.c_float * 2)]


def make_section(plane, half_width=0.0, mode="point", window=None):
    """A VrSection; mode by name ("point", "max", "min", "mean") or number, a missing window is {0, 0} (the transfer function)."""
    sec = VrSection()
    for i in range(4):
        sec.plane[i] = float(plane[i])
    sec.half_width = float(half_width)
    sec.mode = SECTION_MODES[mode] if isinstance(mode, str) else int(mode)
    sec.window[0], sec.window[1] = (0.0, 0.0) if window is None else (float(window[0]), float(window[1]))
    return sec


DEPTH_FIRST, DEPTH_PEAK, DEPTH_MEAN = 0, 1, 2
DEPTH_MODES = {"first": DEPTH_FIRST, "peak": DEPTH_PEAK, "mean": DEPTH_MEAN}
PICK_MAX = 256


class VrDepth(C.Structure):
    """vr_depth: the accumulated alpha a FIRST surface lies at, and the mode (DEPTH_*)"""
    _fields_ = [("opacity", C.c_float), ("mode", C.c_uint32)]


class VrDepthOut(C.Structure):
    """vr_depth_out: the three float buffers of a depth frame; value and alpha may be NULL"""
    _fields_ = [("depth", C.c_void_p), ("value", C.c_void_p), ("alpha", C.c_void_p)]


class VrPick(C.Structure):
    """vr_pick: what a depth frame stores at one pixel, with the model-space position and the continuous voxel index of a hit"""
    _fields_ = [("hit", C.c_uint32), ("k", C.c_float), ("position", C.c_float * 3), ("voxel", C.c_float * 3), ("value", C.c_float), ("alpha", C.c_float)]


def make_depth(opacity, mode="first"):
    """A VrDepth; mode by name ("first", "peak", "mean") or number."""
    d = VrDepth()
    d.opacity = float(opacity)
    d.mode = DEPTH_MODES[mode] if isinstance(mode, str) else int(mode)
    return d


LABEL_COUNT = 256
TF2D_ROWS_MAX = 8              # VR_TF2D_ROWS_MAX
GRADIENT_BINS_MAX = 32         # VR_GRADIENT_BINS_MAX


class VrLabelEntry(C.Structure):
    """vr_label_entry: what a segment does to a sample's classified colour — the straight colour (0..1), how far it replaces the transfer
    function's (mix 0 keeps it, 1 replaces it) and the factor on the sample (opacity 0 hides the segment)"""
    _fields_ = [("colour", C.c_float * 3), ("mix", C.c_float), ("opacity", C.c_float)]


def make_label_entry(colour=(0.0, 0.0, 0.0), mix=0.0, opacity=1.0):
    """A VrLabelEntry; the defaults are the identity entry."""
    e = VrLabelEntry()
    for i in range(3):
        e.colour[i] = float(colour[i])
    e.mix, e.opacity = float(mix), float(opacity)
    return e


FUSE_MODES = {"sum": 0, "over": 1}      # VR_FUSE_SUM, VR_FUSE_OVER


class VrFusion(C.Structure):
    """vr_fusion: how the two fields of a fused frame meet in a sample — the mode and a weight per field, both in 0..1"""
    _fields_ = [("mode", C.c_uint32), ("weight_a", C.c_float), ("weight_b", C.c_float), ("reserved", C.c_uint32)]


def make_fusion(weight_a=1.0, weight_b=1.0, mode="sum"):
    """A VrFusion; mode "sum", "over" or the number.  Weights outside 0..1 and unknown numbers are the ABI's to refuse (VR_ERR_INVALID)."""
    f = VrFusion()
    f.mode = FUSE_MODES[mode] if isinstance(mode, str) else int(mode)
    f.weight_a, f.weight_b, f.reserved = float(weight_a), float(weight_b), 0
    return f


class VrVolumeInfo(C.Structure):
    _fields_ = [("dim_x", C.c_uint32), ("dim_y", C.c_uint32), ("dim_z", C.c_uint32), ("bytes_per_voxel", C.c_uint32),
                ("layout", C.c_uint32), ("brick_copies", C.c_uint32), ("brick_copies_wanted", C.c_uint32), ("brick_planes", C.c_uint32),
                ("linear_resident", C.c_uint32), ("run_copy", C.c_uint32), ("linear_bytes", C.c_uint64), ("bricked_bytes", C.c_uint64),
                ("copies", C.c_uint32), ("copies_in_policy", C.c_uint32), ("copies_refused", C.c_uint32),
                ("build_ms", C.c_float * 13), ("upload_ms", C.c_float)]


class VrRunAlignedInfo(C.Structure):
    _fields_ = [("flavour", C.c_uint32), ("last_flavour", C.c_uint32), ("copies", C.c_uint32), ("copies_refused", C.c_uint32),
                ("bytes", C.c_uint64), ("build_ms", C.c_float * 2)]


class VrTiming(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("total_ms", C.c_float), ("launches", C.c_uint64), ("kernel_ms_sum", C.c_double),
                ("kernel_ms_max", C.c_float), ("total_ms_max", C.c_float)]


class VrLaunchInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("layout", "brick_plane", "lane_map", "phase_x", "phase_y", "clamp_fetch", "tiles_x", "tiles_y",
                                          "ordered", "straddle_permille", "column_voxels", "column_shade_pairs", "shadowed")]


def library_path():
    """In-tree libvr_hip.so; VR_HIP_LIB selects another build of the same library (A/B runs of kernel variants)."""
    return os.environ.get("VR_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvr_hip.so")


_lib = None


def lib():
    """Loads libvr_hip.so once.  Raises (never falls back) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Loaded first, the
    # dynamic linker resolves libvr_hip.so's dependency on that SONAME to the SAME object, so device pointers, streams
    # and events are shared with torch.  Loaded the other way round the process ends up with two runtimes and the
    # second one finds no device.
    import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing — build it with `make -C volume-rendering_amd/csrc` "
                          f"(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    P = C.POINTER
    vp, u32, u64, f32p = C.c_void_p, C.c_uint32, C.c_uint64, P(C.c_float)
    sig = {
        "vr_hip_version": (C.c_char_p, []),
        "vr_hip_create": (C.c_int, [C.c_int, P(vp)]),
        "vr_hip_destroy": (None, [vp]),
        "vr_hip_last_error": (C.c_char_p, [vp]),
        "vr_hip_set_window": (C.c_int, [vp, u32, u32]),
        "vr_hip_set_transfer_fn": (C.c_int, [vp, vp, vp]),
        "vr_hip_set_volume": (C.c_int, [vp, vp, u32, u32, u32, u32]),
        "vr_hip_set_volume_device": (C.c_int, [vp, vp, u32, u32, u32, u32]),
        "vr_hip_set_layout": (C.c_int, [vp, u32]),
        "vr_hip_set_wide_addressing": (C.c_int, [vp, u32]),
        "vr_hip_set_tile_mapping": (C.c_int, [vp, C.c_int32, u32, u32]),
        "vr_hip_set_brick_plane": (C.c_int, [vp, C.c_int32]),
        "vr_hip_set_column_copy": (C.c_int, [vp, u32]),
        "vr_hip_set_run_flavour": (C.c_int, [vp, u32]),
        "vr_hip_run_aligned_info": (C.c_int, [vp, P(VrRunAlignedInfo)]),
        "vr_hip_set_tile_scheduling": (C.c_int, [vp, u32]),
        "vr_hip_set_clip": (C.c_int, [vp, P(VrClip)]),
        "vr_hip_set_shadow": (C.c_int, [vp, P(VrShadow)]),
        "vr_hip_download_shadow": (C.c_int, [vp, vp, u64, P(u32)]),
        "vr_hip_shadow_builds": (C.c_int, [vp, P(u64), f32p]),
        "vr_hip_set_lighting": (C.c_int, [vp, P(VrLighting)]),
        "vr_hip_lighting_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_set_preintegration": (C.c_int, [vp, u32]),
        "vr_hip_preint_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_download_tf_integral": (C.c_int, [vp, f32p]),
        "vr_hip_last_launch": (C.c_int, [vp, P(VrLaunchInfo)]),
        "vr_hip_read_tile_costs": (C.c_int, [vp, vp, u32, P(u32), P(u32)]),
        "vr_hip_render": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_render_device": (C.c_int, [vp, P(VrParams), vp, vp]),
        "vr_hip_render_mip": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_render_mip_device": (C.c_int, [vp, P(VrParams), vp, vp]),
        "vr_hip_render_iso": (C.c_int, [vp, P(VrParams), P(VrIso), vp, vp]),
        "vr_hip_render_iso_device": (C.c_int, [vp, P(VrParams), P(VrIso), vp, vp, vp]),
        "vr_hip_render_backdrop": (C.c_int, [vp, P(VrParams), P(VrBackdrop), vp]),
        "vr_hip_render_backdrop_device": (C.c_int, [vp, P(VrParams), P(VrBackdrop), vp, vp]),
        "vr_hip_render_hybrid": (C.c_int, [vp, P(VrParams), P(VrIso), vp, vp]),
        "vr_hip_render_hybrid_device": (C.c_int, [vp, P(VrParams), P(VrIso), vp, vp, vp]),
        "vr_hip_backdrop_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_render_section": (C.c_int, [vp, P(VrParams), P(VrSection), vp, vp]),
        "vr_hip_render_section_device": (C.c_int, [vp, P(VrParams), P(VrSection), vp, vp, vp]),
        "vr_hip_render_section_in_volume": (C.c_int, [vp, P(VrParams), P(VrSection), vp, vp]),
        "vr_hip_render_section_in_volume_device": (C.c_int, [vp, P(VrParams), P(VrSection), vp, vp, vp]),
        "vr_hip_section_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_render_depth": (C.c_int, [vp, P(VrParams), P(VrDepth), P(VrDepthOut)]),
        "vr_hip_render_depth_device": (C.c_int, [vp, P(VrParams), P(VrDepth), P(VrDepthOut), vp]),
        "vr_hip_pick": (C.c_int, [vp, P(VrParams), P(VrDepth), u32, P(u32), P(VrPick)]),
        "vr_hip_depth_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_set_labels": (C.c_int, [vp, vp, u32, u32, u32]),
        "vr_hip_set_labels_device": (C.c_int, [vp, vp, u32, u32, u32]),
        "vr_hip_set_label_table": (C.c_int, [vp, P(VrLabelEntry), u32]),
        "vr_hip_render_labelled": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_render_labelled_device": (C.c_int, [vp, P(VrParams), vp, vp]),
        "vr_hip_labelled_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_set_tf2d": (C.c_int, [vp, vp, u32, C.c_float, vp]),
        "vr_hip_render_tf2d": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_render_tf2d_device": (C.c_int, [vp, P(VrParams), vp, vp]),
        "vr_hip_tf2d_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_gradient_histogram": (C.c_int, [vp, u32, C.c_float, vp, f32p]),
        "vr_hip_set_second_volume": (C.c_int, [vp, vp, u32, u32, u32, u32]),
        "vr_hip_set_second_volume_device": (C.c_int, [vp, vp, u32, u32, u32, u32]),
        "vr_hip_set_second_transfer_fn": (C.c_int, [vp, vp, vp]),
        "vr_hip_render_fused": (C.c_int, [vp, P(VrParams), P(VrFusion), vp]),
        "vr_hip_render_fused_device": (C.c_int, [vp, P(VrParams), P(VrFusion), vp, vp]),
        "vr_hip_fused_frames": (C.c_int, [vp, P(u64)]),
        "vr_hip_timing": (C.c_int, [vp, P(VrTiming)]),
        "vr_hip_timing_reset": (C.c_int, [vp]),
        "vr_hip_volume_minmax": (C.c_int, [vp, vp, P(u32), f32p, f32p]),
        "vr_hip_volume_histogram": (C.c_int, [vp, vp, f32p]),
        "vr_hip_generate_volume": (C.c_int, [vp, u32, u32, u32, u32]),
        "vr_hip_download_volume": (C.c_int, [vp, vp, u64]),
        "vr_hip_device_info": (C.c_int, [vp, C.c_char_p, C.c_size_t, P(u32), P(u64)]),
        "vr_hip_volume_info": (C.c_int, [vp, P(VrVolumeInfo)]),
        "vr_hip_release_linear_copy": (C.c_int, [vp]),
        "vr_hip_prepare": (C.c_int, [vp, u32]),
        "vr_hip_download_copy": (C.c_int, [vp, u32, vp, u64, vp]),
        "vr_hip_multi_create": (C.c_int, [C.c_int, P(C.c_int), P(vp)]),
        "vr_hip_multi_destroy": (None, [vp]),
        "vr_hip_multi_last_error": (C.c_char_p, [vp]),
        "vr_hip_multi_count": (C.c_int, [vp]),
        "vr_hip_multi_context": (vp, [vp, C.c_int]),
        "vr_hip_multi_transport": (C.c_char_p, [vp]),
        "vr_hip_multi_set_window": (C.c_int, [vp, u32, u32]),
        "vr_hip_multi_set_transfer_fn": (C.c_int, [vp, vp, vp]),
        "vr_hip_multi_set_clip": (C.c_int, [vp, P(VrClip)]),
        "vr_hip_multi_set_shadow": (C.c_int, [vp, P(VrShadow)]),
        "vr_hip_multi_set_lighting": (C.c_int, [vp, P(VrLighting)]),
        "vr_hip_multi_set_preintegration": (C.c_int, [vp, u32]),
        "vr_hip_multi_set_volume": (C.c_int, [vp, vp, u32, u32, u32, u32]),
        "vr_hip_multi_generate_volume": (C.c_int, [vp, u32, u32, u32, u32]),
        "vr_hip_multi_render": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_multi_render_device": (C.c_int, [vp, P(VrParams), vp]),
        "vr_hip_multi_timing": (C.c_int, [vp, f32p, f32p]),
        "vr_hip_multi_render_device_async": (C.c_int, [vp, P(VrParams), vp, vp]),
        "vr_hip_multi_sync": (C.c_int, [vp]),
        "vr_hip_multi_prepare": (C.c_int, [vp, u32]),
        "vr_hip_multi_band_map": (None, [u32, u32, u32, P(u32), P(u32)]),
        "vr_hip_multi_default_band_rows": (u32, [u32, u32]),
        "vr_host_benchmark_view": (C.c_int, [u32, u32, u32, f32p, C.c_float, P(VrView)]),
        "vr_host_benchmark_view_index": (C.c_int, [u32, u32, u32, P(VrView)]),
        "vr_host_raycaster_set_volume": (C.c_int, [vp, u32, u32, u32, vp]),
        "vr_host_raycaster_reset_transfer_fn": (None, []),
        "vr_host_raycaster_set_base_transfer_fn": (C.c_int, [vp]),
        "vr_host_raycaster_change_ray_step": (None, [C.c_float, C.c_int]),
        "vr_host_raycaster_change_ray_threshold": (None, [C.c_float, C.c_int]),
        "vr_host_raycaster_change_light_intensity": (None, [C.c_float, C.c_int]),
        "vr_host_raycaster_set_esl": (None, [C.c_int]),
        "vr_host_raycaster_reset_ray_step": (None, []),
        "vr_host_raycaster_get": (C.c_int, [P(VrParams), vp, vp, vp, vp]),
        "vr_host_render_frame": (C.c_int, [C.c_int, u32, P(VrView), vp]),
        "vr_host_set_clip": (None, [P(VrClip)]),
        "vr_host_set_shadow": (None, [P(VrShadow)]),
        "vr_host_load_model": (C.c_int, [C.c_char_p, P(u32)]),
        "vr_host_set_raw_dims": (None, [u32, u32, u32, u32]),
        "vr_host_model_voxels": (vp, []),
        "vr_host_model_histogram": (None, [f32p]),
        "vr_host_quantize": (C.c_int, [vp, u32, u32, u32, C.c_int, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)      # AttributeError here = the library does not export what the headers declare
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = None  # filled lazily by tests from the headers
