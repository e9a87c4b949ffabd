/*
 * vr_hip.h — C ABI of the MI355X-native volume raycaster (libvr_hip.so).
 *
 * This is the drop-in boundary for ONE path of MiroBeno/Volume-Rendering: what happens below
 * `Renderer::render_volume()` and the three `Renderer::set_*()` calls (reference VolumeRendering/Renderer.h:13-28),
 * i.e. the work the reference does in GPURenderer1.cu:65-112, GPURenderer23.cu:55-81 and GPURenderer4.cu:89-153.
 * The host C++ mirror of the reference interface (volume-rendering_amd/csrc/host/Renderer.h, class HipRenderer)
 * is the intended caller; INTEGRATION.md shows the few lines a maintainer of the reference adds.
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no C++/torch types; every entry point returns 0 on success and a
 *     non-zero vr_status otherwise; nothing exits the process or throws (the reference's cuda_safe_call
 *     exit(EXIT_FAILURE) policy, cuda_utils.h:21-31, is deliberately NOT reproduced below the ABI);
 *   - one opaque vr_ctx per GPU, no globals (the reference keeps everything in statics, Renderer.h:39-43);
 *   - a context is not thread-safe (neither is the reference);
 *   - there is NO CPU fallback: without a usable HIP device vr_hip_create() fails with VR_ERR_NO_DEVICE;
 *   - a frame depends on the context's CURRENT state alone — the last value every setter below was given, and what the text of a setter
 *     says it drops — never on the calls that led there (tests/test_gpu_session.py).  Where a frame is refused for more than one reason,
 *     VR_ERR_INVALID (arguments, or a state under which the call can never succeed: the sampling mode, pre-integration) is reported
 *     before the VR_ERR_NOT_READY of a missing state (labels, the 2-D table, the second field or its function).
 */
#ifndef VR_HIP_H
#define VR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Reference constants, RaycasterBase.h:12-16 */
#define VR_TF_SIZE          128   /* TF_SIZE: entries of the transfer function (float4 each, premultiplied) */
#define VR_TF_RATIO         2     /* TF_RATIO = 256 / TF_SIZE */
#define VR_ESL_VOLUME_DIMS  32    /* ESL_VOLUME_DIMS: empty-space-leaping grid is 32^3 blocks */
#define VR_ESL_VOLUME_SIZE  1024  /* ESL_VOLUME_SIZE: 32^3 bits = 1024 uint32 words */
#define VR_ESL_MIN_BLOCK    8     /* ESL_MIN_BLOCK_SIZE */

typedef enum vr_status {
	VR_OK               = 0,
	VR_ERR_INVALID      = 1,  /* NULL / out-of-range argument; same value the reference returns (CPURenderer.cpp:44-45) */
	VR_ERR_NO_DEVICE    = 2,
	VR_ERR_ALLOC        = 3,  /* device allocation failed (reference: GPURenderer1.cu:91-95 returns 1) */
	VR_ERR_HIP          = 4,  /* any other HIP runtime error; see vr_hip_last_error() */
	VR_ERR_NOT_READY    = 5   /* render before set_window / set_transfer_fn / set_volume */
} vr_status;

typedef enum vr_sampling {
	VR_SAMPLE_NEAREST   = 0,  /* Model::sample_data (ModelBase.h:17-23) + transfer_fn[sample / TF_RATIO] (CPURenderer.cpp:31):
	                             semantics of CPURenderer and GPURenderer1/2/3 */
	VR_SAMPLE_TRILINEAR = 1,  /* GPURenderer4 semantics (GPURenderer4.cu:76-77,91-99,136-141): trilinear volume fetch with
	                             normalised coordinates + clamp addressing, linearly filtered transfer function;
	                             interpolation weights in full fp32 */
	VR_SAMPLE_TRILINEAR_Q8 = 2 /* the same, with the three volume weights and the transfer-function weight rounded to 8
	                             fractional bits (rint(w * 256) / 256) before use — the published definition of the linear
	                             filtering GPURenderer4's tex3D / tex1D calls run on ("9-bit fixed point with 8 bits of
	                             fractional value"): what the texture unit of renderer 4 computes, as far as it is specified */
} vr_sampling;

/* How the render paths keep the volume in HBM.  VR_LAYOUT_LINEAR: every sampling mode reads the reference's linear array.
 * VR_LAYOUT_BRICKED (default): TRILINEAR reads quad or run bricks, NEAREST reads voxel bricks (one voxel per element in brick
 * order) — copies built from the linear array on first use (vr_hip_prepare builds them ahead of time).
 * All layouts give bit-identical images; the choice is speed only. */
typedef enum vr_layout {
	VR_LAYOUT_LINEAR  = 0,    /* x-fastest linear array exactly as Model::data (ModelBase.h:18-22) */
	VR_LAYOUT_BRICKED = 1     /* default: "quad bricks" — every element packs the 2x2 (x,y) voxel neighbourhood of a slice into
	                             one aligned word, stored in 8x8x8-element bricks: a trilinear sample is two aligned loads
	                             and the cache-line footprint no longer depends on the view direction
	                             (4x the voxel bytes in HBM per copy, up to three copies for 1-byte voxels — vr_hip_set_brick_plane;
	                             volume-rendering_amd/csrc/vr_device.h) */
} vr_layout;

/* struct View, ViewBase.h:14-21 (dims widened to 32 bit, bool -> uint32) */
typedef struct vr_view {
	uint32_t width, height;     /* View::dims */
	float origin[3];
	float direction[3];
	float right_plane[3];
	float up_plane[3];
	float light_pos[3];
	uint32_t perspective;       /* 0 = orthogonal, 1 = perspective */
} vr_view;

/* The by-value part of struct Raycaster (RaycasterBase.h:20-30) that travels with every render_volume() call,
 * plus the sampling mode and the screen-space partition used for multi-GPU rendering. */
typedef struct vr_params {
	vr_view  view;
	float    ray_step;          /* Raycaster::ray_step */
	float    ray_threshold;     /* Raycaster::ray_threshold (early ray termination) */
	uint32_t esl;               /* Raycaster::esl (empty space leaping on/off) */
	uint32_t esl_block_dims;    /* Raycaster::esl_block_dims (voxels per ESL block edge) */
	float    esl_block_size[3]; /* Raycaster::esl_block_size (block edge in model space) */
	float    light_kd;          /* Raycaster::light_kd */
	uint32_t sampling;          /* vr_sampling */
	/* Screen-space partition. The output buffer holds out_rows rows of out_width pixels (RGBA8, row-major, y-up):
	 *   out[ly * out_width + lx]  <-  frame pixel (x0 + lx, gy)
	 *   gy = ((ly / band_rows) * band_stride + band_first) * band_rows + ly % band_rows
	 * Whole frame: x0 = 0, out_width = width, out_rows = height, band_rows = height, band_stride = 1, band_first = 0.
	 * Rank r of n (interleaved bands of b rows): band_rows = b, band_stride = n, band_first = r.
	 * Pixels with gy >= height stay cleared. */
	uint32_t x0, out_width, out_rows;
	uint32_t band_rows, band_stride, band_first;
} vr_params;

typedef struct vr_ctx vr_ctx;

/* Per-frame statistics filled in by vr_hip_timing(). */
typedef struct vr_timing {
	float    kernel_ms;     /* hipEvent time of the ray-march kernel of the last render (on the render's stream) */
	float    total_ms;      /* clear + parameter upload + kernel (+ D2H copy for vr_hip_render), the reference's timed region
	                           (VolR.cpp:109-111, GPURenderer1.cu:107-110) */
	uint64_t launches;      /* ray-march launches since the last vr_hip_timing_reset() */
	double   kernel_ms_sum; /* sum of kernel_ms over those launches */
	float    kernel_ms_max; /* the longest of those launches (the reference's Profiler keeps sum and max, Profiler.cpp:69-72) */
	float    total_ms_max;  /* the longest vr_hip_render call (kernel + D2H) since the reset */
} vr_timing;

/* ---- lifetime: replaces GPURenderer1::GPURenderer1 / ~GPURenderer1 (GPURenderer1.cu:17-28) ---- */
int  vr_hip_create(int device, vr_ctx **out);
void vr_hip_destroy(vr_ctx *ctx);
const char *vr_hip_last_error(const vr_ctx *ctx);           /* never NULL */

/* ---- Renderer::set_window_buffer(View) — GPURenderer1.cu:74-84: (re)allocates the device framebuffer ---- */
int vr_hip_set_window(vr_ctx *ctx, uint32_t width, uint32_t height);

/* ---- Renderer::set_transfer_fn(Raycaster) — GPURenderer1.cu:65-72: uploads the premultiplied TF (128 x float4)
 *      AND the ESL bit-volume (1024 words; bit set = block empty) ---- */
int vr_hip_set_transfer_fn(vr_ctx *ctx, const float *tf_premult_rgba, const uint32_t *esl_bits);

/* ---- Renderer::set_volume(Model) — GPURenderer1.cu:86-97: copies the host voxels to HBM.
 *      bytes_per_voxel 1 (reference) or 2 (build-side extension, little-endian u16); sizes are 64-bit inside. ---- */
int vr_hip_set_volume(vr_ctx *ctx, const void *host_voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                      uint32_t bytes_per_voxel);
/* same, source already in device memory (x-fastest, unpadded) */
int vr_hip_set_volume_device(vr_ctx *ctx, const void *dev_voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                             uint32_t bytes_per_voxel);

/* Layout policy for the TRILINEAR copy of the volume (default VR_LAYOUT_BRICKED).  Takes effect immediately for the
 * resident volume (rebuilds or drops the bricked copy) and for later set_volume calls.  No reference counterpart. */
int vr_hip_set_layout(vr_ctx *ctx, uint32_t layout);

/* Testing aid: makes every later frame use one of the two 64-bit addressing paths that volumes beyond 1024^3 / 4 GiB need
 * (BASELINE config 5), so that they can be parity-tested on small volumes: 1 = index arithmetic without tables (dims above
 * 2048), 2 = address tables with 64-bit z offsets (dims up to 2048), 0 = automatic; + 4 = clamp the fetch coordinates of
 * every sample, which only views very far from the volume or very long ray steps need; + 8 = NEAREST does not use the
 * scaled-domain address chain that volumes with power-of-two edges get.  Images are identical either way. */
int vr_hip_set_wide_addressing(vr_ctx *ctx, uint32_t force);

/* Which of the up to three brick copies the TRILINEAR fetch reads — they differ in the plane, (x,y) / (x,z) / (y,z), that the
 * 16-byte chunks of the brick order cover (volume-rendering_amd/csrc/vr_device.h): -1 = per view, the plane perpendicular to
 * the view's dominant axis (default); 0, 1, 2 = always that plane (where the copy exists: 1-byte voxels, edges up to 1024,
 * else (x,y)); 3 / 4 = the "run bricks", copies in which the two slices of a sample along z / along y are 8 adjacent bytes (one
 * gather per sample), which per-view selection uses for every view whose lane quads cannot be chunk-aligned; 5 = 2-byte volumes read
 * their oct bricks (one 16-byte element per cell) for EVERY view — per-view selection uses them for orthogonal views with at most
 * one cell per pixel and the quad bricks otherwise; 6 = BOTH run copies in one launch, chosen per screen tile — what per-view
 * selection does for full-march frames of views that are not along a volume axis: which copy is cheaper depends on the cube face
 * a tile's rays enter through, so frames 0 - 3 of a parameter set run on one copy each (twice, the second time recording what every
 * tile cost) and from frame 4 on every tile reads the copy that was cheaper for it — here for every view; 7 = both copies on
 * alternating tiles (no measurement; parity tests); 8 = the column windows (VR_COPY_COL_*) along the view's major axis for EVERY orthogonal
 * full-march frame — per-view selection reads them only when the view runs along a volume axis; 9 = never (the round-3 choice for
 * those views).  Speed only; testing and tuning aid.  No reference counterpart. */
int vr_hip_set_brick_plane(vr_ctx *ctx, int32_t plane);

/* Which copy the TRILINEAR frames that take the column march read: 0 = the windows of 16 plain voxels (VR_COPY_COLV_*, 1 byte per
 * voxel) wherever the host can bound the cell columns of every 8x8-pixel wave to 64 (default; the quad-element windows otherwise);
 * 1 = always the quad-element windows (VR_COPY_COL_*, 16/3 bytes per voxel; the round-4 march); 2 = as 0, but without the second
 * copy described next.  In mode 0 a LIT frame (light_kd > 0.01) that marches over the voxel windows fetches its shading samples —
 * positions a few cells off the ray, outside what the wave holds — from the quad-element windows of the same axis, one 8-byte load
 * instead of eight byte loads: the first such frame along an axis builds that copy too (16/3 bytes per voxel: 5.35 GiB per axis at
 * 1024^3 beside the 1 GiB of voxel windows; all three axes visited: about 16 GiB more than mode 2 holds).  Where it cannot be had
 * (the half-of-the-HBM rule of vr_hip_prepare, an allocation failure, the linear array released) the frame shades by byte loads as
 * in mode 2, with the same image; vr_launch_info::column_shade_pairs tells which.  Unlit frames never ask for it.  Mode 2 is the
 * memory opt-out.  Speed only; A/B and testing aid.  No reference counterpart. */
int vr_hip_set_column_copy(vr_ctx *ctx, uint32_t mode);

/* Which pixels of a 4x4-pixel block share a lane quad, and where the tile grid starts: speed only, images are identical.
 * lane_map -1 = chosen per frame from the view (default); else (lane order) + 4 * (wave shape): order 0 = 4 pixels along screen x,
 * 1 = along screen y, 2 = 2x2-pixel blocks; wave shape 0 = 8x8 pixels per wavefront, 1 = 16 wide x 4 high, 2 = 4 wide x 16 high;
 * phase_x / phase_y (0..7) shift the tile grid left / down (ignored when lane_map is -1).  Testing and tuning aid
 * (tests force every combination and compare the images).  No reference counterpart. */
int vr_hip_set_tile_mapping(vr_ctx *ctx, int32_t lane_map, uint32_t phase_x, uint32_t phase_y);

/* In which order the screen tiles of a frame are started: 1 (default) = measured-cost order — the first frame with a given set of
 * parameters records what every tile cost (its longest wavefront), a small kernel behind it sorts the tiles, and later frames with
 * the same parameters start their most expensive tiles first, so that a few long tiles (rays that probe along a block face, deep
 * rays next to early-terminated ones) no longer form the tail of the frame; applied only while empty-space leaping or early ray
 * termination is on (the full march has no tail).  0 = tile number = workgroup id, always.  Placement only: images are identical.
 * 2 = as 0, and every frame leaves a COST MAP behind (profiling): vr_hip_read_tile_costs copies the last frame's tiles_x * tiles_y
 * values — duration of the tile's workgroup, from its start to the end of its last wavefront, in units of 64 shader-clock cycles, row
 * major from the bottom-left tile of the kernel's tile grid (32x16-pixel tiles; 32x32 on the 1024-thread paths); `host_out` NULL
 * only reports the grid.  Waits for the context's frames.
 * No reference counterpart (its 16x16 blocks are started in grid order, GPURenderer1.cu:81-82,108). */
int vr_hip_set_tile_scheduling(vr_ctx *ctx, uint32_t mode);
int vr_hip_read_tile_costs(vr_ctx *ctx, uint32_t *host_out, uint32_t capacity, uint32_t *tiles_x, uint32_t *tiles_y);

/* ---- Renderer::render_volume(uchar4 *buffer, Raycaster r) ----
 * vr_hip_render: `host_rgba` is a HOST pointer of out_width*out_rows*4 bytes (renderer ids 0-2 in the reference,
 *   VolR.cpp:76-87; GPURenderer1.cu:107-110 = clear + kernel + D2H).  Synchronous.  A frame of unpartitioned rows (band_stride 1) of
 *   at least 1 MiB is rendered as two row slices on two streams of the context, so that the first slice's copy to the host runs while
 *   the second still renders; the bytes written are the same (VR_HOST_SLICES=1: one launch + one copy).
 * vr_hip_render_device: `dev_rgba` is a DEVICE pointer (renderer ids 3-4, GPURenderer23.cu:72-81) — clear + kernel on
 *   `stream` (a hipStream_t).  NULL means the context's OWN non-blocking stream, which is not ordered against the legacy
 *   default stream: a caller that fills or reads `dev_rgba` on another stream must pass that stream (or synchronise itself).
 *   Asynchronous with respect to the host.
 * Return 0 ok / VR_ERR_INVALID on NULL arguments like the reference (GPURenderer1.cu:101-102). */
int vr_hip_render(vr_ctx *ctx, const vr_params *params, uint8_t *host_rgba);
int vr_hip_render_device(vr_ctx *ctx, const vr_params *params, void *dev_rgba, void *stream);

/* ---- maximum-intensity projection (MIP): the second projection next to the front-to-back composite above.  No reference counterpart. ----
 * Per pixel:
 *  1. the ray is View::get_ray + Raycaster::intersect exactly as in vr_hip_render; a miss leaves the pixel cleared (0,0,0,0);
 *  2. the samples are those of the march with leaping off: `while (kx <= ky) { sample at kx; kx += ray_step; }` — kx, ky from intersect,
 *     kx accumulated by repeated addition, the position formed from kx for every sample.  Nothing below changes this sequence;
 *  3. VR_SAMPLE_NEAREST: m = the integer maximum of the raw voxels Model::sample_data returns (its unfused arithmetic); the colour is
 *     transfer_fn[s8 / VR_TF_RATIO] with s8 = m for 1-byte voxels and m >> 8 for 2-byte voxels;
 *  4. VR_SAMPLE_TRILINEAR / _Q8: m = the float maximum of the interpolated RAW value (texel coordinates fma(k, A, B), the lerps of the
 *     TRILINEAR mode, Q8 with rounded weights), starting at 0; the colour is the linearly filtered transfer-function lookup of m with the
 *     arithmetic of a composited sample's lookup (Q8: rounded weight);
 *  5. the pixel is write_color(colour): the premultiplied entry as it is stored.  No shading, no compositing: ray_threshold, light_kd and
 *     light_pos are ignored;
 *  6. x0, out_width, out_rows and band_* partition the frame as in vr_hip_render.
 * params.esl selects EXACT acceleration.  0: every sample is fetched, no ray stops early.  Otherwise the kernel may skip the fetch of a
 * sample whose value provably cannot exceed the ray's current m — by the maximum of the sample's ESL block (NEAREST) or of the 3x3x3
 * blocks around it (TRILINEAR: a sample's cell can lie one voxel outside its block), in the block grid vr_hip_volume_minmax reports for
 * the resident volume (params.esl_block_* and the ESL bits of vr_hip_set_transfer_fn are not used) — and may stop a ray whose m has
 * reached the maximum of the volume.  Only fetches are skipped; kx += ray_step runs for every sample up to the point where the ray
 * stops, so images with esl on and off are identical byte for byte.  The block maxima are derived on the device from the min/max scan
 * by the first such frame after a set_volume* / generate_volume and kept until the next; vr_hip_release_linear_copy derives them
 * before it frees the array they are scanned from.
 * Return values, NULL conventions and VR_ERR_NOT_READY as for vr_hip_render / vr_hip_render_device (the transfer function must be set);
 * the brick copy a frame reads (voxel bricks for NEAREST, quad or oct bricks for TRILINEAR, the linear array under VR_LAYOUT_LINEAR) is
 * built on first use; vr_hip_set_wide_addressing and vr_hip_set_tile_mapping apply; frames are counted by vr_hip_timing and described
 * by vr_hip_last_launch.  vr_hip_render_mip is one launch and one copy to the host. */
int vr_hip_render_mip(vr_ctx *ctx, const vr_params *params, uint8_t *host_rgba);
int vr_hip_render_mip_device(vr_ctx *ctx, const vr_params *params, void *dev_rgba, void *stream);

/* ---- shaded isosurface with depth: the third projection.  No reference counterpart. ----
 * The first point along every ray where the interpolated field reaches `level`, shaded from the field's gradient, and the depth of that
 * point.  Per pixel:
 *  1. Ray.  View::get_ray + Raycaster::intersect exactly as in vr_hip_render.  A miss leaves the pixel (0,0,0,0) and the depth -1.
 *  2. Sample sequence.  The samples are those of the march with leaping off: `while (kx <= ky) { sample at kx; kx += ray_step; }`, k
 *     accumulated by repeated addition.  Nothing below changes this sequence; it is the MIP frame's sequence.
 *  3. Field value and first hit.  v(k) is the TRILINEAR (or _Q8) interpolated RAW value at texel coordinates fma(k, A, B), with the A, B
 *     and lerps of the TRILINEAR mode.  The first hit is the first sample i with v(k_i) >= level.  No such sample: pixel (0,0,0,0),
 *     depth -1.
 *  4. Refinement.  If i = 0 the hit is k* = k_0: the surface is already reached where the ray enters the cube, and nothing is refined.
 *     Otherwise lo = k_(i-1), the accumulated k of the previous sample, whose value is < level by construction, and hi = k_i; `refine`
 *     times: `mid = 0.5f * (lo + hi); if (v(mid) >= level) hi = mid; else lo = mid;`.  Then k* = hi.
 *  5. Colour.  base = the linearly filtered transfer-function lookup of `level` with the arithmetic of a composited sample's lookup
 *     (_Q8: rounded weight): the premultiplied entry as stored, so an isosurface at level l and a MIP pixel whose maximum is l have the
 *     same base colour.
 *  6. Shading.  If light_kd <= 0.01f then f = 1 and no gradient is fetched.  Otherwise, with (xb, yb, zb) = fma(k*, A, B), the gradient
 *     is central differences one texel apart, clamp addressing as everywhere: gx = (v(xb + 1, yb, zb) - v(xb - 1, yb, zb)) * half.x,
 *     likewise gy and gz; half = N/2 takes the texel gradient to model space, where the cube is [-1,1]^3 whatever the dims.
 *     gg = fma(gz, gz, fma(gy, gy, gx * gx)).  If gg is not > 0 then s = 0.  Else, with pt = origin + direction * k* (fused),
 *     dl = light_pos - pt, il = rsqrt_nr(fma(dl.z, dl.z, fma(dl.y, dl.y, dl.x * dl.x))) and dot = fma(gz, dl.z, fma(gy, dl.y, gx * dl.x)):
 *     s = fminf(fabsf((dot * rsqrt_nr(gg)) * il), 1.0f), rsqrt_nr the Newton reciprocal square root of the TRILINEAR mode's light vector.
 *     The shading is two-sided: a surface seen from inside the bright region is lit like one seen from outside.
 *     f = fma(light_kd, s, 1.0f - light_kd).
 *  7. Pixel.  write_color(base.x * f, base.y * f, base.z * f, base.w).  ray_threshold is ignored.
 *  8. Depth.  Where a buffer is given, it holds out_width * out_rows floats laid out exactly like the RGBA buffer (x0, out_width,
 *     out_rows, band_*): k* for a surface pixel and -1.0f for every other pixel, rows with gy >= height included.  k is the parameter of
 *     the pixel's own ray: position = origin + direction * k with the origin and direction get_ray gives that pixel — the perspective
 *     direction is NOT normalised, so k is not a distance there.  The RGBA bytes do not depend on whether depth is asked for.
 *  9. params.esl selects EXACT acceleration.  0: every sample of the march is fetched.  Otherwise the kernel may skip the fetch of a
 *     march sample whose bound is below `level`: the 3x3x3-dilated maximum of the sample's block in the grid of vr_hip_volume_minmax,
 *     widened exactly as a MIP frame widens it for TRILINEAR / _Q8 and 2-byte voxels.  As for MIP, params.esl_block_* and the ESL bits
 *     of vr_hip_set_transfer_fn are not used.  k += ray_step still runs for every sample; bisection and gradient fetches are never
 *     skipped.  Images and depths with esl on and off are identical byte for byte.
 * 10. Errors.  VR_SAMPLE_NEAREST -> VR_ERR_INVALID (a gradient-shaded first hit is defined on the interpolated field: the two TRILINEAR
 *     modes are supported).  A NULL iso, a non-finite level, or refine > 16 -> VR_ERR_INVALID.  Everything else follows
 *     vr_hip_render_mip: the NULL conventions, VR_ERR_NOT_READY without volume or transfer function, the guards on ray_step.
 * 11. Shared behaviour with MIP frames.  The frame reads what a MIP frame of the same view and sampling reads — quad bricks with the
 *     per-view chunk plane, oct bricks for 2-byte voxels where a MIP frame takes them, the linear array under VR_LAYOUT_LINEAR —, never
 *     a run copy or a column window; the copy is built on first use.  vr_hip_set_wide_addressing, vr_hip_set_tile_mapping,
 *     vr_hip_set_layout and vr_hip_set_brick_plane(5) apply; frames are counted by vr_hip_timing and described by vr_hip_last_launch.
 *     vr_hip_render_iso is one launch plus one copy to the host per buffer.  It renders on a single device: the vr_hip_multi_* path
 *     has no isosurface. */
typedef struct vr_iso {
	float    level;    /* in RAW voxel units: 0..255 for 1-byte voxels, 0..65535 for 2-byte voxels; must be finite */
	uint32_t refine;   /* bisection steps after the first hit, 0..16 */
} vr_iso;
int vr_hip_render_iso(vr_ctx *ctx, const vr_params *params, const vr_iso *iso, uint8_t *host_rgba, float *host_depth /* may be NULL */);
int vr_hip_render_iso_device(vr_ctx *ctx, const vr_params *params, const vr_iso *iso, void *dev_rgba, void *dev_depth /* may be NULL */, void *stream);

/* ---- clip region for all three projections: a crop box and a cutting plane.  No reference counterpart. ----
 * The clip is context state, like the layout knobs: it applies to every later composite (vr_hip_render*), MIP (vr_hip_render_mip*) and
 * isosurface (vr_hip_render_iso*) frame of the context, and through the per-device contexts to vr_hip_multi_* frames
 * (vr_hip_multi_set_clip).  NULL switches clipping off, which is the default; without a clip every frame is what it was.  vr_params and
 * every other struct keep their size and layout.  Clipping only narrows each ray's segment [kx, ky] before the march.  Per pixel, right
 * after View::get_ray and Raycaster::intersect have produced origin, dir, kx, ky and reported a hit:
 *  1. Box.  d' = dir with exact zeros replaced by 0.00001f, as inside intersect.  k1 = (box_min - origin) / d' and
 *     k2 = (box_max - origin) / d' per component, IEEE division; kxb = the max over the axes of min(k1, k2), kyb = the min over the axes of
 *     max(k1, k2), min / max being the `a < b ? a : b` / `a > b ? a : b` of flmin / flmax in the association order of intersect.  Then
 *     kx = flmax(kx, kxb) and ky = flmin(ky, kyb).  A box equal to [-1,1]^3 therefore changes no bit.
 *  2. Plane, from the unreplaced dir.  dn = fma(n.z, dir.z, fma(n.y, dir.y, n.x * dir.x)) and, with o = origin,
 *     on = fma(n.z, o.z, fma(n.y, o.y, fma(n.x, o.x, d))).  dn > 0: kx = flmax(kx, -on / dn).  dn < 0: ky = flmin(ky, -on / dn).
 *     dn == 0: the ray is kept unchanged if on >= 0, else it is a miss.  (All four plane members 0: dn == 0 and on == 0, no plane.)
 *  3. Hit test.  The ray is a hit iff (kx < ky) && (ky > 0).  A miss is treated exactly as an intersect miss: pixel (0,0,0,0), isosurface
 *     depth -1.
 *  4. March.  Everything after that is the frame's own definition applied to the clipped segment.  Composite: the leaping loop and the
 *     accumulation `while (kx <= ky)` start at the clipped kx.  MIP / isosurface: the sample sequence is
 *     `k = kx; while (k <= ky) { ...; k += ray_step; }` from the clipped kx.  Isosurface: a hit at sample 0 is k* = kx — a cut through the
 *     region at or above the level shows the cut face, shaded from the field's gradient there; depth stays the parameter of the pixel's
 *     own ray.  Exact acceleration is per sample and untouched: the ESL bits, the transparent-sample shortcut, the MIP / isosurface block
 *     bounds, early termination.
 *  5. Guards.  The two guards on ray_step (ky + step > ky, the cap on the number of steps) look at the UNCLIPPED segment, which contains
 *     the clipped one; they cannot bind for parameters the entry points accept.
 *  6. Errors.  VR_ERR_INVALID for a non-finite member and for box_min[i] >= box_max[i].  A box that misses the cube is valid: every
 *     frame is empty.
 *  7. What a clipped frame reads.  The linear array, quad, voxel or oct bricks — never a run copy or a column window, whatever
 *     vr_hip_set_brick_plane forces (3, 4, 6, 7, 8 fall back to the quad copy of plane (x,y)): vr_launch_info::layout is never 2, 3, 6
 *     or 7 for a clipped frame.  Setting a clip that differs from the current one forgets the cached tile mappings and recorded tile
 *     orders (placement only; they are keyed by vr_params alone). */
typedef struct vr_clip {
	float box_min[3], box_max[3]; /* model space; the cube is [-1,1]^3 whatever the dims */
	float plane[4];               /* kept half-space: n.x*x + n.y*y + n.z*z + d >= 0; all four 0 = no plane */
} vr_clip;
int vr_hip_set_clip(vr_ctx *ctx, const vr_clip *clip);       /* NULL = clipping off (the default) */

/* ---- light-source shadows for composite frames: a light grid and one more filtered fetch per dense sample.  No reference counterpart. ----
 * The reference's lighting (Raycaster::shade) is one extra sample 0.01 units towards view.light_pos: a local gradient cue.  A shadow makes the
 * dense part of the volume darken what lies behind it as seen from the light.  It is context state, like the clip: NULL switches it off, which
 * is the default; without a shadow, or with strength 0, every frame is what it was, byte for byte.  vr_params and every other struct keep
 * their size and layout.
 * Shadow volume.  S^3 bytes q (S = dims), x fastest, built on the context's stream — synchronous, like a brick copy — by the first composite
 * frame, or vr_hip_download_shadow, that finds it missing or stale.  It goes stale on a vr_hip_set_shadow whose struct differs from the
 * current one in more than `strength` (q does not depend on it: a change of the strength alone keeps the grid; after NULL there is no
 * current one: setting the same shadow again rebuilds), on vr_hip_set_volume* / vr_hip_generate_volume, on vr_hip_set_transfer_fn, and on a vr_hip_set_clip that differs from the
 * current clip.  Per node (i, j, k):
 *  1. Position.  n = fma((float) i, 2.0f / (float) (S - 1), -1.0f) per axis.
 *  2. Light vector.  d = light_pos - n, len2 = fma(d.z, d.z, fma(d.y, d.y, d.x * d.x)).  If !(len2 > 0) then T = 1.  Otherwise
 *     il = rsqrt_nr(len2) (the Newton reciprocal square root of the TRILINEAR mode's light vector), u = d * il (three plain multiplies),
 *     dist = len2 * il.
 *  3. Segment.  intersect(n, u) exactly as for a view ray (exact zeros of u replaced by 0.00001f, kx = flmax(kx, 0)); a miss gives T = 1.
 *     On a hit, if a clip is set, steps 1-3 of the clip contract are applied to (n, u, kx, ky); a miss there also gives T = 1.
 *     t_end = flmin(ky, dist).
 *  4. March.  T = 1; t = flmax(kx, 0) + step (one plain IEEE add; kx is 0 without a clip).  while (t <= t_end): raw = the TRILINEAR (or _Q8,
 *     by `sampling`) interpolated RAW value at texel coordinates fma(t, A, B) with A = u * half and B = fma(n, half, half - 0.5f) — the
 *     composite's own A and B, built from the node instead of the ray origin; a = the .w of the linearly filtered transfer-function lookup of
 *     raw with the arithmetic of a composited sample's lookup (_Q8: rounded weight); T = T * (1.0f - a); if (T < cutoff) { T = 0; break; }
 *     t += step.  The loop also carries an explicit bound of ceil(2 sqrt(3) / step) + 2 steps, which cannot bind for accepted parameters.
 *     NOTHING is opacity-corrected for step != ray_step (that takes a powf, which CPU and GPU do not share bit for bit): for shadows as
 *     dense as the frame sees them, choose step = ray_step.
 *  5. Store.  q = (uint8_t) (T * 255.0f + 0.5f), product and sum rounded separately.
 * Shadowed composite frame.  vr_hip_render / vr_hip_render_device (and vr_hip_multi_* through the per-device contexts) composite as before
 * with one addition: for a sample whose looked-up colour has c.w > 0.05f — whatever light_kd is — the colour is scaled AFTER the diffuse
 * term is added and BEFORE the sample is accumulated: c.xyz *= f with f = fma(strength * (1.0f / 255.0f), Tq, 1.0f - strength).  Tq is the
 * trilinear interpolation of q at the sample's model-space point pt = march_point(origin, dir, k), the point the lighting already forms; per
 * axis v = fmed3(fma(pt, hs, hs), 0, S - 1) with hs = 0.5f * (S - 1), i = min((uint32_t) v, S - 2), w = v - (float) i; lerps fma(w, b - a, a)
 * along x, then y, then z; full fp32 weights in both sampling modes.  Alpha, leaping, the transparent-sample shortcut and early termination
 * see the same alphas and are untouched.
 * Other behaviour.  VR_SAMPLE_NEAREST composite frames under a shadow return VR_ERR_INVALID (the builder and the factor are defined on the
 * interpolated field: the isosurface's precedent).  MIP and isosurface frames IGNORE the shadow (shadowed isosurfaces are a follow-up).  A
 * shadowed frame reads what a clipped frame reads — the linear array, quad bricks with the per-view plane, or oct bricks —, never a run copy
 * or a column window; vr_launch_info::shadowed tells.  Setting or changing the shadow — but for its strength alone — forgets the cached
 * tile mappings and recorded orders, as vr_hip_set_clip does.  light_pos is independent of view.light_pos (the wrappers set both).
 * Errors.  VR_ERR_INVALID for a non-finite member, dims outside 2..256, step < 1/4096, strength outside [0,1], cutoff outside [0,1), a
 * sampling other than VR_SAMPLE_TRILINEAR / _Q8.  vr_hip_download_shadow: VR_ERR_NOT_READY without a shadow, volume or transfer function,
 * VR_ERR_INVALID for a short buffer, or a NULL one with a capacity (NULL with capacity 0 only reports *dims_out).  vr_hip_shadow_builds counts the builds of the context (testing aid: an identical
 * vr_hip_set_shadow does not rebuild) and reports the hipEvent time of the last one. */
typedef struct vr_shadow {
	float    light_pos[3];  /* model space; the cube is [-1,1]^3.  Independent of view.light_pos (the wrappers set both) */
	uint32_t dims;          /* S: nodes per edge of the light grid, 2..256 */
	float    step;          /* march step towards the light, in model units; finite, >= 1/4096 */
	float    strength;      /* 0..1: 0 = frames equal unshadowed frames byte for byte */
	float    cutoff;        /* 0 <= cutoff < 1: a light ray whose transmittance falls below it is black */
	uint32_t sampling;      /* VR_SAMPLE_TRILINEAR or VR_SAMPLE_TRILINEAR_Q8: how the builder samples the volume */
} vr_shadow;
int vr_hip_set_shadow(vr_ctx *ctx, const vr_shadow *shadow);      /* NULL = off (the default) */
int vr_hip_download_shadow(vr_ctx *ctx, uint8_t *host_out, uint64_t capacity, uint32_t *dims_out); /* S^3 bytes, x fastest; builds if stale */
int vr_hip_shadow_builds(vr_ctx *ctx, uint64_t *builds_out, float *last_build_ms_out);              /* either may be NULL */

/* ---- gradient lighting for composite frames: Blinn-Phong from the gradient of the interpolated field.  No reference counterpart. ----
 * The reference's lighting is a cue — (raw_l - raw) * kd added to all three channels: it has no normal and no highlight, and cannot tell
 * "facing the light" from "steeper".  A lighting shades every dense sample from the central-difference gradient of the field, the
 * isosurface's (step 6 there), with an ambient, a two-sided diffuse and a white specular term.  It is context state, like the clip and the
 * shadow: NULL switches it off, which is the default; without a lighting every frame is what it was, byte for byte.  vr_params and every
 * other struct keep their size and layout.
 * Lit composite frame.  vr_hip_render / vr_hip_render_device (and vr_hip_multi_* through the per-device contexts) composite as before with one
 * replacement: the block that adds the reference's cue is not run and params.light_kd is IGNORED.  For a sample whose looked-up colour has
 * c.w > 0.05f, with (xb, yb, zb) = fma(k, A, B) the sample's texel coordinates and pt = march_point(origin, dir, k) the model-space point
 * the march already forms for it:
 *  1. Gradient.  gx = (v(xb + 1, yb, zb) - v(xb - 1, yb, zb)) * half.x, likewise gy and gz; v is the TRILINEAR (or _Q8, by params.sampling)
 *     interpolated RAW value with clamp addressing; gg = fma(gz, gz, fma(gy, gy, gx * gx)).  If !(gg > 0) the sample is left as looked up: a
 *     plateau has no surface to light.
 *  2. Light.  ig = rsqrt_nr(gg); dl = view.light_pos - pt; ll = fma(dl.z, dl.z, fma(dl.y, dl.y, dl.x * dl.x)).  If !(ll > 0) then
 *     sd = sp = 0.  Otherwise il = rsqrt_nr(ll), dot = fma(gz, dl.z, fma(gy, dl.y, gx * dl.x)), sd = fminf(fabsf((dot * ig) * il), 1.0f):
 *     two-sided, as the isosurface is.
 *  3. Highlight.  iv = rsqrt_nr(fma(dir.z, dir.z, fma(dir.y, dir.y, dir.x * dir.x))) from the pixel's own unnormalised dir;
 *     h = fma(-dir, iv, dl * il) per axis (the product rounded on its own); hh = fma(h.z, h.z, fma(h.y, h.y, h.x * h.x)).  If !(hh > 0) then
 *     sp = 0.  Otherwise sp = fminf(fabsf((fma(gz, h.z, fma(gy, h.y, gx * h.x)) * ig) * rsqrt_nr(hh)), 1.0f), then sp = sp * sp repeated
 *     shininess_log2 times.  There is no powf: CPU and GPU do not share one bit for bit (the shadow builder's reasoning).
 *  4. Colour.  m = fma(diffuse, sd, ambient); spec = (specular * sp) * c.w — the highlight is white and premultiplied;
 *     c.x = fma(c.x, m, spec), likewise y and z.  c.w is untouched: leaping, the transparent-sample shortcuts and early termination see the
 *     same alphas, and the alpha bytes of a lit frame equal the unlit frame's.
 *  5. Shadow.  The factor of vr_hip_set_shadow, where one is set, scales c.xyz after step 4, as its contract says: the two compose.
 * Consequences.  { 1, 0, 0, n } gives the bytes of the same frame with light_kd = 0: fma(c, 1, (0 * sp) * c.w) = c.  Samples with
 * c.w <= 0.05f are never lit, as in the reference.
 * Other behaviour.  VR_SAMPLE_NEAREST composite frames under a lighting return VR_ERR_INVALID (the isosurface's and the shadow's precedent).
 * MIP and isosurface frames IGNORE the lighting.  A lit frame reads what a clipped frame reads — the linear array, quad bricks with the
 * per-view plane, or oct bricks —, never a run copy or a column window: vr_launch_info::layout is then 0, 1 or 5.  Setting a lighting that
 * differs from the current one forgets the cached tile mappings and recorded orders, as vr_hip_set_shadow does.
 * Errors.  VR_ERR_INVALID for a non-finite member, a coefficient outside [0, 1], shininess_log2 > 10.  vr_hip_lighting_frames counts the
 * composite frames this context launched on the gradient-lit kernels (testing aid). */
typedef struct vr_lighting {
	float    ambient;         /* ka, 0..1 */
	float    diffuse;         /* kd, 0..1 */
	float    specular;        /* ks, 0..1 */
	uint32_t shininess_log2;  /* n, 0..10: the specular term is raised to the power 2^n by n squarings */
} vr_lighting;                /* 16 bytes */
int vr_hip_set_lighting(vr_ctx *ctx, const vr_lighting *lighting);      /* NULL = off (the default): the reference's cue */
int vr_hip_lighting_frames(vr_ctx *ctx, uint64_t *frames_out);          /* testing aid: composite frames launched on the gradient-lit kernels */

/* ---- pre-integrated (slab) classification for composite frames, in the integral-function form.  No reference counterpart. ----
 * The reference classifies a sample by one transfer-function lookup at its value: whatever the transfer function holds between the values of
 * two consecutive samples is never seen, a thin peak shows as rings and missed shells, and whether a ray catches it depends on the phase of
 * its samples.  Pre-integration classifies the SLAB between two consecutive samples by the mean of the piecewise-linear transfer function
 * over it.  It is context state, like the clip, the shadow and the lighting: off by default, and without it every frame is what it was, byte
 * for byte.  vr_params and every other struct keep their size and layout.
 * Integral table.  vr_hip_set_transfer_fn builds K, 128 x float4, on the host from the 128 premultiplied entries it is given and uploads it
 * next to them: K[0] = 0 and K[i + 1] = fmaf(0.5f, tf[i] + tf[i + 1], K[i]) per channel for i = 0..126, in that order (the explicit fmaf).
 * K(t), for a transfer-function coordinate t in [0, 127]: i = min((uint32_t) t, 126), w = t - (float) i,
 * K(t) = fmaf(w, fmaf(0.5f * w, tf[i + 1] - tf[i], tf[i]), K[i]) per channel — full fp32 weights in both TRILINEAR modes (the shadow factor's
 * precedent).  No expf and no powf: CPU and GPU do not share one bit for bit.
 * Slab composite frame.  vr_hip_render / vr_hip_render_device (and vr_hip_multi_* through the per-device contexts) composite as before with one
 * replacement, the looked-up colour c of a sample.  tb is the sample's clamped transfer-function coordinate, formed as before:
 * fmed3(fma(raw, tf_scale, -0.5f), 0, 127).  tp is the tb of the PREVIOUS sample of the accumulation loop; for the loop's first sample — the
 * first at or after the clipped and leapt kx; there is no leaping inside the accumulation loop — tp = tb.  d = tb - tp.
 *  - Narrow slab, !(fabsf(d) >= 0.5f): c is the ordinary filtered lookup of the frame's sampling mode (in _Q8 the weight is rounded) at
 *    tm = 0.5f * (tp + tb).  With d == 0 this is the point-classified lookup, bit for bit.
 *  - Wide slab, otherwise: r = 1.0f / d by IEEE division and c = (K(tb) - K(tp)) * r per channel, the difference and the product rounded
 *    separately.
 * Everything after the lookup is unchanged and sees this c: the c.w > 0.05f dense test, the reference's cue (with the sample's own raw and
 * raw_l), the shadow factor, the gradient lighting (steps 1-5 of its contract), the accumulation and early termination.
 * Exact shortcuts.  K(t) is exactly 0 for t <= tf_zero_below, so a sample contributes exactly nothing when both tp and tb are below it; a
 * sample whose tb is below it but whose tp is not is NOT transparent.
 * Other behaviour.  VR_SAMPLE_NEAREST composite frames under pre-integration return VR_ERR_INVALID (the isosurface's, the shadow's and the
 * lighting's precedent).  MIP and isosurface frames IGNORE the state.  The shadow builder ignores it: light rays stay point classified.  A
 * slab frame reads what a clipped frame reads — the linear array, quad bricks with the per-view plane, or oct bricks —, never a run copy or a
 * column window: vr_launch_info::layout is then 0, 1 or 5.  Setting a state that differs from the current one forgets the cached tile
 * mappings and recorded orders, as vr_hip_set_lighting does.  There is no opacity correction: the table is the one of the frame's own step.
 * Errors.  VR_ERR_INVALID for on > 1.  vr_hip_preint_frames counts the composite frames this context launched on the slab kernels and
 * vr_hip_download_tf_integral returns K as uploaded, 512 floats (testing aids). */
int vr_hip_set_preintegration(vr_ctx *ctx, uint32_t on);               /* 0 = off (the default), 1 = slab classification; other values VR_ERR_INVALID */
int vr_hip_preint_frames(vr_ctx *ctx, uint64_t *frames_out);           /* testing aid: composite frames launched on the slab kernels */
int vr_hip_download_tf_integral(vr_ctx *ctx, float *host_out512);      /* testing aid: K, 128 x float4; VR_ERR_NOT_READY without a transfer function */

/* ---- backdrop: a composite frame over an opaque layer, and the hybrid of isosurface and volume.  No reference counterpart. ----
 * A backdrop frame is a composite frame (with the context's clip, shadow, lighting and pre-integration as vr_hip_render_device sees them)
 * whose rays stop at the depth of an opaque RGBA8 layer and whose accumulated colour is blended over the layer's: a rasterised tool, a slice
 * plane or a background image behind the volume, or — the hybrid — the isosurface of the same volume inside it.  It is a per-call argument,
 * not context state: without it every frame is what it was, byte for byte.  vr_params and every other struct keep their size and layout.
 * Layers.  rgba: out_width * out_rows RGBA8 words, premultiplied; depth: as many floats, k of the pixel's own ray — the unit of the
 * isosurface frame's depth buffer.  Both are partitioned by x0, out_width, out_rows, band_* exactly as the output: pixel (lx, ly) reads element
 * ly * out_width + lx.
 * Per pixel, behind View::get_ray, Raycaster::intersect and steps 1-3 of the clip contract (a backdrop frame always runs the clip's
 * arithmetic, under the identity clip when none is set, which changes no bit):
 *  1. d = depth[pixel].  The pixel HAS A SURFACE iff d >= 0.0f, an ordered compare: -1, any negative value and NaN mean no surface, +inf is a
 *     surface behind everything (the background image).
 *  2. No surface: the pixel is exactly what the frame without a backdrop stores; the layer's colour word is ignored.
 *  3. Surface: ky = flmin(ky, d) (intersect's flmin), and the ray is a hit iff it was one and (kx < ky) && (ky > 0), the clip's test.  Everything
 *     after that is the composite's own definition on the narrowed segment: the leaping loop and the accumulation loop `while (kx <= ky)` — a
 *     sample at k == d is composited —, the classification, the cue, the shadow, the lighting, the slab, early termination.  The two guards
 *     on ray_step look at the unnarrowed segment, as under a clip.
 *  4. Pixel of a surface ray, b the layer's colour word: if the ray is a miss, or leaping leaves kx > ky, the pixel is b bit for bit.  Otherwise,
 *     per channel, bf = ((float) byte + 0.5f) * (1.0f / 256.0f) (both exact), t = 1.0f - acc.w, o = fmaf(bf, t, acc) and the pixel is
 *     write_color(o).  With acc == 0 that is b again; t is not clamped, and early termination changes nothing here.
 *  5. In place: dev_rgba may be the layer's rgba — a pixel reads its own layer elements and writes only its own output element.
 * Hybrid.  vr_hip_render_hybrid_device is by definition vr_hip_render_iso_device with the same params and iso into dev_rgba and dev_depth (a
 * context-owned depth buffer when dev_depth is NULL), followed on the same stream by vr_hip_render_backdrop_device in place.  The isosurface
 * frame sees clip, light_kd and esl as it always does and ignores shadow, lighting and pre-integration; the composite pass sees all of them.
 * The depth returned is the isosurface's.  The context-owned buffers (the depth, and the staging of the layers for the host entry points)
 * are allocated on first use and grown, never per frame; the host entry points are one upload per layer into one staging buffer (backdrop) or none
 * (hybrid), the launches and one copy back per buffer.
 * What such a frame reads.  What a clipped frame reads — vr_launch_info::layout is 0, 1 or 5 —, never a run copy or a column window.  Its
 * tiles start in grid order: it neither uses nor records a measured tile order and leaves the cached mappings alone (the caches are keyed
 * by vr_params and the layer changes per frame; this affects placement only).  Single device: the vr_hip_multi_* path has no backdrop.
 * Errors.  VR_ERR_INVALID for a NULL struct or member and for VR_SAMPLE_NEAREST: the hybrid's surface is defined on the interpolated field
 * and the kernels cover the TRILINEAR modes; a NEAREST backdrop is not provided.  VR_ERR_NOT_READY, the NULL conventions and everything else
 * as for vr_hip_render_device (the hybrid: and as for vr_hip_render_iso_device).  vr_hip_backdrop_frames counts the composite frames this
 * context launched on the backdrop kernels (testing aid). */
typedef struct vr_backdrop {
	const void *rgba;   /* out_width * out_rows RGBA8 words, premultiplied, laid out exactly like the frame's output buffer */
	const void *depth;  /* out_width * out_rows floats, same layout: k of the pixel's own ray (the isosurface frame's depth) */
} vr_backdrop;          /* 16 bytes */
int vr_hip_render_backdrop_device(vr_ctx *ctx, const vr_params *params, const vr_backdrop *dev, void *dev_rgba, void *stream);
int vr_hip_render_backdrop(vr_ctx *ctx, const vr_params *params, const vr_backdrop *host, uint8_t *host_rgba);
int vr_hip_render_hybrid_device(vr_ctx *ctx, const vr_params *params, const vr_iso *iso, void *dev_rgba, void *dev_depth /* may be NULL */, void *stream);
int vr_hip_render_hybrid(vr_ctx *ctx, const vr_params *params, const vr_iso *iso, uint8_t *host_rgba, float *host_depth /* may be NULL */);
int vr_hip_backdrop_frames(vr_ctx *ctx, uint64_t *frames_out);         /* testing aid: composite frames launched on the backdrop kernels */

/* ---- section: an oblique slice through the interpolated field and its thick-slab forms, with depth.  No reference counterpart. ----
 * A section frame is the planar reformat of a volume viewer: the field on the plane n.x*x + n.y*y + n.z*z + d = 0 (POINT), or the maximum,
 * minimum or mean of the field over the slab |n.x*x + n.y*y + n.z*z + d| <= h around it (slab MIP, MinIP, the X-ray-like average), coloured
 * through the transfer function or a grey window.  It writes the depth layer of the isosurface frame, so it is the second producer of the
 * layer a backdrop frame takes: vr_hip_render_section_in_volume is the slice inside the translucent volume, as the hybrid is for the
 * isosurface.  The section is a per-call argument, not context state: vr_params and every other struct keep their size and layout.
 * Per pixel:
 *  1. Ray.  View::get_ray + Raycaster::intersect exactly as in vr_hip_render, then steps 1-3 of the clip contract under the context's clip.
 *     As a backdrop frame does, a section frame always runs the clip's arithmetic, under the identity clip when none is set, which changes no
 *     bit.  A miss gives pixel (0,0,0,0) and depth -1.
 *  2. Plane, from the unreplaced dir, with the clip's two expressions: dn = fma(n.z, dir.z, fma(n.y, dir.y, n.x * dir.x)),
 *     on = fma(n.z, o.z, fma(n.y, o.y, fma(n.x, o.x, d))).  dn == 0 is a miss in every mode: a ray parallel to the section has no section
 *     point.  Otherwise kc = -on / dn by IEEE division.
 *  3. Segment.  POINT: the pixel is a hit iff the ray was one and (kx <= kc) && (kc <= ky), ordered compares; the segment becomes [kc, kc].
 *     Thick modes: ka = ((-h) - on) / dn, kb = (h - on) / dn, kx = flmax(kx, flmin(ka, kb)), ky = flmin(ky, flmax(ka, kb)) (intersect's
 *     flmin / flmax), and the ray is a hit iff it was one and (kx < ky) && (ky > 0), the clip's test.
 *  4. Samples.  k = kx; while (k <= ky) { v(k); k += ray_step; } — the MIP frame's sequence on the narrowed segment —, v the TRILINEAR (or
 *     _Q8) interpolated RAW value at fma(k, A, B) with the A, B and lerps of the TRILINEAR mode.  POINT is the one sample v(kc).  The two
 *     guards on ray_step look at the unnarrowed segment, as under a clip.  params.esl, ray_threshold, light_kd and light_pos are ignored:
 *     every sample is fetched.
 *  5. Value.  MAX: m = 0; m = raw > m ? raw : m.  MIN: m = +inf; m = raw < m ? raw : m.  MEAN: s = 0; s = s + raw in sample order, plain adds,
 *     n counted; the value is s / (float) n by IEEE division (a hit has n >= 1).  POINT: v(kc).
 *  6. Colour.  window == {0, 0}: the linearly filtered transfer-function lookup of the value with the arithmetic of a MIP pixel's lookup
 *     (_Q8: rounded weight); the pixel is write_color of the premultiplied entry as stored.  Otherwise inv = 1.0f / (hi - lo), formed once on
 *     the host, g = fmed3((value - lo) * inv, 0, 1) with the difference and the product rounded separately, and the pixel is
 *     write_color(g, g, g, 1.0f): an opaque grey, which is what the backdrop wants as a layer.
 *  7. Depth.  The layout of the isosurface's depth buffer.  POINT: kc.  Thick modes: the narrowed kx, the slab's front face.  Every other
 *     pixel: -1, rows with gy >= height included.  The RGBA bytes do not depend on whether depth is asked for.
 *     Raycaster::intersect clamps kx at 0, so a hit has kc >= kx >= 0: a section point behind a camera inside the cube is a miss, and the depth
 *     of every hit reads as a surface to a backdrop frame (d >= 0.0f).
 *  8. In volume.  vr_hip_render_section_in_volume_device is by definition vr_hip_render_section_device into dev_rgba and dev_depth (the
 *     context-owned depth buffer of the hybrid when dev_depth is NULL), followed on the same stream by vr_hip_render_backdrop_device in
 *     place.  The section pass ignores shadow, lighting and pre-integration; the composite pass sees them.  The depth returned is the
 *     section's.  The host entry point mirrors vr_hip_render_hybrid.
 *  9. What it reads.  What a clipped MIP frame of that view and sampling reads — quad bricks with the per-view plane, oct bricks for 2-byte
 *     voxels, or the linear array —, never a run copy or a column window; vr_hip_set_wide_addressing, vr_hip_set_tile_mapping,
 *     vr_hip_set_layout and vr_hip_set_brick_plane apply.  Tiles start in grid order.  Frames are counted by vr_hip_timing, described by
 *     vr_hip_last_launch and counted by vr_hip_section_frames (testing aid).  Single device: the vr_hip_multi_* path has no section.
 * 10. Errors.  VR_ERR_INVALID for a NULL section, a non-finite member, a normal of three zeros, mode > 3, half_width < 0, POINT with
 *     half_width != 0, a thick mode with half_width == 0, a window that is neither {0, 0} nor hi > lo, and VR_SAMPLE_NEAREST: a section is
 *     defined on the interpolated field.  Everything else as for vr_hip_render_iso*. */
typedef enum vr_section_mode { VR_SECTION_POINT = 0, VR_SECTION_MAX = 1, VR_SECTION_MIN = 2, VR_SECTION_MEAN = 3 } vr_section_mode;
typedef struct vr_section {
	float    plane[4];    /* n.x, n.y, n.z, d: the section is n.x*x + n.y*y + n.z*z + d = 0, model space, cube [-1,1]^3 */
	float    half_width;  /* h: the slab is |n.x*x + n.y*y + n.z*z + d| <= h (model units for a unit normal); 0 for POINT */
	uint32_t mode;        /* vr_section_mode */
	float    window[2];   /* lo, hi in RAW voxel units: grey window; both 0 = colour by the transfer function */
} vr_section;             /* 32 bytes */
int vr_hip_render_section(vr_ctx *ctx, const vr_params *params, const vr_section *section, uint8_t *host_rgba, float *host_depth /* may be NULL */);
int vr_hip_render_section_device(vr_ctx *ctx, const vr_params *params, const vr_section *section, void *dev_rgba, void *dev_depth /* may be NULL */, void *stream);
int vr_hip_render_section_in_volume(vr_ctx *ctx, const vr_params *params, const vr_section *section, uint8_t *host_rgba, float *host_depth /* may be NULL */);
int vr_hip_render_section_in_volume_device(vr_ctx *ctx, const vr_params *params, const vr_section *section, void *dev_rgba, void *dev_depth /* may be NULL */, void *stream);
int vr_hip_section_frames(vr_ctx *ctx, uint64_t *frames_out);          /* testing aid: section frames launched */

/* ---- depth frames of the composite, and pixel picking.  No reference counterpart. ----
 * A depth frame says where along its ray the thing a composite pixel shows lies: the depth k of the pixel's own ray, the interpolated raw
 * value there and the pixel's final alpha, three float buffers laid out exactly like the isosurface's depth buffer (x0, out_width, out_rows,
 * band_*; rows with gy >= height hold -1 / -1 / 0).  The composite's alpha depends only on the sampling mode, the clip, the leaping and the
 * classification — the shadow's and the lighting's contracts both leave alpha untouched — so one alpha-only march mirrors every composite
 * frame a context can launch.  The depth buffer is the third producer of the layer a backdrop frame takes.  vr_depth is a per-call argument,
 * not context state: vr_params and every other struct keep their size and layout.
 *  1. Ray.  get_ray + intersect, then steps 1-3 of the clip contract under the context's clip; with no clip set the identity clip, always
 *     run, as for backdrop and section frames.  A miss gives depth -1, value -1, alpha 0.
 *  2. Leaping.  The composite's leaping loop in front of the accumulation loop, under params.esl with the ESL bits of
 *     vr_hip_set_transfer_fn.  If no sample is left (kx > ky) the pixel is a miss.
 *  3. Accumulation.  For each sample of `while (kx <= ky)`, in this order: raw = the TRILINEAR (or _Q8) value at fma(kx, A, B); a = the .w of
 *     the sample's classified colour — the filtered lookup, or under vr_hip_set_preintegration(1) the slab colour of that contract (narrow /
 *     wide, tp of the previous sample of this loop, the first sample's tp = tb), the composite's arithmetic —; t = 1 - acc, g = a * t (a plain
 *     product, rounded on its own), acc = fmaf(a, t, acc); the record of step 4; `if (acc > ray_threshold) break;` — the sample that
 *     terminates the ray is recorded —; kx += ray_step.
 *  4. Record.  FIRST: at the first sample whose acc >= opacity (ordered compare, acc after the update) depth = that kx, value = that raw.
 *     PEAK: `if (g > best) { best = g; depth = kx; value = raw; }`, best starting at 0: the first of equal peaks wins, a sample with g = 0
 *     never does.  MEAN: sg = sg + g; sk = fmaf(kx, g, sk); sv = fmaf(raw, g, sv), in sample order.
 *  5. Result.  FIRST / PEAK: as recorded, else depth -1 and value -1.  MEAN: if sg > 0, depth = sk / sg and value = sv / sg (IEEE division),
 *     else -1 / -1.  alpha = the final acc, in every mode.
 *  6. Consequences.  map_float_int(alpha, 256) is the alpha byte of the composite frame of the same params under the same clip and
 *     pre-integration state, whatever shadow and lighting are set.  Every surface has depth >= 0: the depth buffer is a valid backdrop layer.
 *  7. What it ignores.  light_kd, light_pos, shadow and lighting.  The two guards on ray_step look at the unclipped segment.
 *  8. Exact acceleration.  The kernel may take the composite's transparent-sample shortcuts (under pre-integration a sample whose tp is above
 *     tf_zero_below is not transparent) and may stop a FIRST ray at its surface when no alpha buffer is asked for.  Results do not depend on
 *     which buffers are asked for.
 *  9. What it reads.  What a clipped MIP frame of that view and sampling reads — linear array, quad or oct bricks, never a run copy or a
 *     column window: vr_launch_info::layout is 0, 1 or 5; vr_hip_set_layout and vr_hip_set_brick_plane apply.  Tiles start in grid order.
 *     Frames are counted by vr_hip_timing, described by vr_hip_last_launch and counted by vr_hip_depth_frames (testing aid).  Single device:
 *     the vr_hip_multi_* path has no depth frame.
 * 10. Errors.  VR_ERR_INVALID for a NULL struct, a NULL depth buffer, mode > 2, a non-finite opacity, an opacity outside [0, 1], FIRST with
 *     opacity 0 (a transparent sample would be a surface), and VR_SAMPLE_NEAREST.  Everything else as for vr_hip_render_iso*.
 * Pick.  out[i] is by definition what a whole-frame depth frame stores at frame pixel (xy[2i], xy[2i+1]) (y up; the partition fields of
 * params are ignored): hit = depth >= 0, and k, value, alpha are that pixel's values.  For a hit, with that pixel's own ray,
 * position = fma(dir, k, origin) per axis and voxel = fma(k, A, B) per axis — a continuous voxel index: voxel i's centre is at i.  Without
 * a hit k = -1, value = -1, position and voxel 0.  Synchronous, on the context's stream.  n = 0 is fine; n > 256, a pixel outside the
 * window or a NULL pointer with n > 0 give VR_ERR_INVALID. */
typedef enum vr_depth_mode { VR_DEPTH_FIRST = 0, VR_DEPTH_PEAK = 1, VR_DEPTH_MEAN = 2 } vr_depth_mode;
typedef struct vr_depth {
	float    opacity;     /* FIRST: the accumulated alpha a surface lies at, (0, 1]; PEAK, MEAN: in [0, 1], not looked at */
	uint32_t mode;        /* vr_depth_mode */
} vr_depth;               /* 8 bytes */
typedef struct vr_depth_out {
	void *depth;          /* out_width * out_rows floats */
	void *value;          /* likewise, or NULL */
	void *alpha;          /* likewise, or NULL */
} vr_depth_out;           /* 24 bytes */
typedef struct vr_pick {
	uint32_t hit;
	float    k;
	float    position[3]; /* model space, cube [-1,1]^3 */
	float    voxel[3];    /* continuous voxel index */
	float    value;       /* raw voxel units */
	float    alpha;
} vr_pick;                /* 40 bytes */
#define VR_PICK_MAX 256
int vr_hip_render_depth_device(vr_ctx *ctx, const vr_params *params, const vr_depth *depth, const vr_depth_out *dev, void *stream);
int vr_hip_render_depth(vr_ctx *ctx, const vr_params *params, const vr_depth *depth, const vr_depth_out *host);
int vr_hip_pick(vr_ctx *ctx, const vr_params *params, const vr_depth *depth, uint32_t n, const uint32_t *xy /* 2n */, vr_pick *out);
int vr_hip_depth_frames(vr_ctx *ctx, uint64_t *frames_out);            /* testing aid: depth frames launched (a pick counts one per query) */

/* ---- label volumes: per-segment colour and visibility for composite frames.  No reference counterpart. ----
 * A second volume of one byte per voxel names the segment a voxel belongs to; a table of 256 entries says what a segment does to the colour
 * the transfer function returns for a sample inside it: tint it, replace it, fade it or hide it.  Two structures of the same density can
 * then differ in colour, and a structure can be removed without a box or a plane.
 *  1. State.  Labels are context state: dx * dy * dz bytes, x fastest, with the dims of the resident volume (other dims: VR_ERR_INVALID; no
 *     volume: VR_ERR_NOT_READY).  The bytes are copied; the host entry is synchronous, the device entry copies on the context's stream.  NULL
 *     drops them.  vr_hip_set_volume*, vr_hip_generate_volume drop them too: vr_hip_render_labelled* then returns VR_ERR_NOT_READY.  The
 *     table survives until it is replaced: entries [0, count) as given, the rest — and all 256 after NULL / 0, and before the first call —
 *     the identity { colour anything, mix 0, opacity 1 }.  Setting labels or a table changes no other frame of the context: every other entry
 *     point ignores both.  Every existing struct keeps its size; the frames are counted by vr_hip_labelled_frames (testing aid).
 *  2. Frame.  The composite frame vr_hip_render_device defines for a TRILINEAR or _Q8 frame under the context's clip (the identity clip when
 *     none is set, always run), gradient lighting and shadow — leaping by params.esl, the cue, early termination, the band and crop
 *     partition — with one insertion, directly behind the filtered lookup c of a sample at tb and in front of the `c.w > 0.05f` test.
 *     (xb, yb, zb) = fma(k, A, B) are the sample's texel coordinates.
 *  3. Nearest label.  ix = (uint32_t) fmed3(xb + 0.5f, 0.0f, (float) (Nx - 1)), the add one plain IEEE add; iy, iz likewise;
 *     l = labels[(iz * Ny + iy) * Nx + ix].
 *  4. Table.  e = table[l].  Per colour channel c.x = fmaf(e.mix, fmaf(e.colour[0], c.w, -c.x), c.x), with the unscaled c.w (c is
 *     premultiplied, colour is straight); then all four channels are multiplied by e.opacity, plain products.
 *  5. Everything behind the insertion sees this c: the dense test, the cue (with the sample's own raw and raw_l), lighting steps 1-5, the
 *     shadow's factor, the accumulation and `acc.w > ray_threshold`.
 *  6. Exact acceleration.  Both transparency shortcuts of the composite stay: c == 0 stays 0 under every entry.  The label of a sample the
 *     wave skips need not be fetched.  A sample whose entry has opacity 0 contributes exactly nothing.
 *  7. Consequences.  (a) With an all-identity table the bytes equal vr_hip_render of the same context state (fmaf(0, x, c) == c, c * 1 == c).
 *     (b) With every opacity 0 the frame is all zero bytes.  (c) One constant label with { mix 0, opacity 0.5 } and no shadow: the bytes equal
 *     the unlabelled frame rendered with every transfer-function entry halved — scaling by a power of two commutes with every rounding of
 *     the lookup.
 *  8. Shadow.  The light grid is built from the unlabelled classification: a hidden segment still casts its shadow.  Label-aware light rays
 *     are a follow-up.
 *  9. Pre-integration.  VR_ERR_INVALID while vr_hip_set_preintegration(1) holds: a slab between two samples with different labels has no
 *     single entry.  A follow-up.
 * 10. What it reads.  The field as a depth frame reads it — linear array, quad or oct bricks, never a run copy or a column window:
 *     vr_launch_info::layout is 0, 1 or 5; vr_hip_set_layout and vr_hip_set_wide_addressing apply.  The labels are read from the linear
 *     array, or — 1-byte voxels in quad bricks behind address tables — from a copy in the 1-byte voxel-brick order of chunk plane (x,y),
 *     built on first use, which the field's own address tables address: such a frame reads the (x,y) quad copy whatever the view.  Tiles
 *     start in grid order.  Frames are counted by vr_hip_timing and described by vr_hip_last_launch.
 * 11. Errors.  VR_ERR_INVALID for VR_SAMPLE_NEAREST, for count > 256, for NULL entries with count > 0, for a table member that is not
 *     finite or outside [0, 1], and while pre-integration is on.  Everything else as for vr_hip_render*.
 * Out of scope: the device list (vr_hip_multi_*), a backdrop under a labelled frame, interpolated label boundaries, labels in MIP,
 * isosurface, section and depth frames. */
#define VR_LABEL_COUNT 256
typedef struct vr_label_entry {
	float colour[3];      /* 0..1, straight (not premultiplied) */
	float mix;            /* 0..1: 0 keeps the transfer function's colour, 1 replaces it by `colour` */
	float opacity;        /* 0..1: scales the sample; 0 hides the segment */
} vr_label_entry;         /* 20 bytes */
int vr_hip_set_labels(vr_ctx *ctx, const uint8_t *host_labels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z);    /* NULL = drop */
int vr_hip_set_labels_device(vr_ctx *ctx, const void *dev_labels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z);
int vr_hip_set_label_table(vr_ctx *ctx, const vr_label_entry *entries, uint32_t count);
int vr_hip_render_labelled(vr_ctx *ctx, const vr_params *params, uint8_t *host_rgba);
int vr_hip_render_labelled_device(vr_ctx *ctx, const vr_params *params, void *dev_rgba, void *stream);
int vr_hip_labelled_frames(vr_ctx *ctx, uint64_t *frames_out);         /* testing aid: labelled frames launched */

/* ---- 2D transfer-function frames: classify by value and gradient magnitude.  No reference counterpart. ----
 * The gradient magnitude of the field is the second classification axis (Levoy 1988; Kniss et al. 2002): material interiors sit at a low
 * gradient magnitude, the boundary between two materials is an arch that reaches a high one at intermediate values.  A table over (value,
 * gradient magnitude) shows boundaries without the solid behind them, and separates two boundaries that cross the same values.
 *  1. State.  `table` is rows * 128 float4, premultiplied: row r is a transfer function of the value in the layout vr_hip_set_transfer_fn
 *     takes.  rows is 2..VR_TF2D_ROWS_MAX.  The table is context state and is copied; NULL drops it.  It survives a volume change, is
 *     independent of the 1-D transfer function, and every other entry point ignores it.  esl_bits are 1024 words, the leaping bits of THIS
 *     table in the format and with the meaning the 1-D function's bits have: the caller builds them from the envelope of step 7.  The call
 *     waits for the context's frames first, as vr_hip_set_transfer_fn does.  Every existing struct keeps its size; the frames are counted
 *     by vr_hip_tf2d_frames (testing aid).
 *  2. Frame.  The composite frame vr_hip_render_device defines for a TRILINEAR or _Q8 frame under the context's clip (the identity clip when
 *     none is set, always run), gradient lighting and shadow — leaping by params.esl on the table's own bits, the cue, early termination, the
 *     band and crop partition — with one replacement: the looked-up colour c of a sample.  (xb, yb, zb) = fma(k, A, B) are the sample's
 *     texel coordinates.
 *  3. Value axis.  raw, tb, i = (uint32_t) (int) tb, i1 = min(i + 1, 127) and w = filter_weight(fract(tb)) are formed as the composite forms
 *     them; w is rounded in _Q8.
 *  4. Gradient.  Exactly step 1 of the lighting contract: the central differences one texel apart of the interpolated raw value, clamp
 *     addressing, times half_x / y / z; gg = fma(gz, gz, fma(gy, gy, gx * gx)); g = gg > 0 ? gg * rsqrt_nr(gg) : 0.  No sqrtf: CPU and GPU
 *     share every bit.  The differences span two texels and are not halved: g is TWICE the length of the model-space gradient (on a ramp
 *     of slope s per voxel along x, g = 2 s half_x), and g_scale is chosen against that g.
 *  5. Row.  tg = fmed3(g * g_scale, 0, rows - 1); j = min((uint32_t) tg, rows - 2); wg = tg - (float) j, full fp32 in both sampling modes
 *     (the shadow factor's precedent).
 *  6. Colour, per channel: c_j = fma(w, T[j][i1] - T[j][i], T[j][i]); c_j1 the same in row j + 1; c = fma(wg, c_j1 - c_j, c_j).  Every
 *     subtraction is rounded on its own.  Everything behind the lookup sees this c: the `c.w > 0.05f` test, the reference's cue when no
 *     lighting is set, lighting steps 2-5 with the gradient of step 4 and not a second one, the shadow's factor, the accumulation and
 *     `acc.w > ray_threshold`.
 *  7. Envelope and exact shortcuts.  E[i] is the per-channel maximum over the rows.  tf_zero_below and the corner test of a tf2d frame are
 *     derived from E exactly as vr_hip_set_transfer_fn derives them from the 1-D function: both transparency shortcuts of the composite
 *     stay exact.  Entry i is g-independent when every row holds the bit patterns of row 0 at i and at i1; then c is row 0's lookup bit for
 *     bit (fma(wg, 0, x) = x), and the gradient of a sample need not be fetched where nothing reads it: no counting lane's entry is
 *     g-dependent and the wave has no lit dense lane.
 *  8. Consequences.  (a) Every row equal to the context's transfer function, with the same ESL bits: the bytes of vr_hip_render under the
 *     same state, for any g_scale.  (b) g_scale = 0: the bytes of vr_hip_render with row 0 as the transfer function.  (c) On a plateau
 *     (gg = 0) only row 0 is seen.  (d) An all-zero table gives a zero frame.
 *  9. Shadow.  The light grid is the context's, built from the 1-D transfer function (the label precedent): a boundary the table hides still
 *     casts the shadow the 1-D function gives it.  A grid built from the 2-D table is a follow-up.
 * 10. What it reads.  What a labelled frame reads — the linear array, quad bricks or oct bricks: vr_launch_info::layout is 0, 1 or 5, tiles
 *     start in grid order and `ordered` is 0; vr_hip_set_layout, vr_hip_set_wide_addressing and vr_hip_set_brick_plane apply.  Frames are
 *     counted by vr_hip_timing and described by vr_hip_last_launch.  Single device only.
 * 11. Errors.  VR_ERR_INVALID for VR_SAMPLE_NEAREST, while pre-integration is on (a slab has no single row), for rows outside 2..8, for a
 *     g_scale or a table member that is not finite or is negative, and for NULL esl_bits with a table.  VR_ERR_NOT_READY for a frame without
 *     a table.  Everything else as for vr_hip_render*.
 * 12. Histogram.  vr_hip_gradient_histogram places the rows: for every voxel of the resident volume, bin = the 1-D histogram's bin (the
 *     byte, or the high byte of a u16); gx = ((float) v(x+1) - (float) v(x-1)) * half_x with indices clamped to the axis, gy and gz likewise
 *     (step 4 at integer texel coordinates, where every filter weight is 0); gg and g as in step 4; tg = fmed3(g * g_scale, 0, g_bins - 1);
 *     row = (uint32_t) (tg + 0.5f); hist[row * 256 + bin] += 1.  Preconditions and errors are vr_hip_volume_histogram's (the linear copy is
 *     needed); g_bins outside 1..VR_GRADIENT_BINS_MAX and a g_scale that is not finite or is negative return VR_ERR_INVALID.  Summed over
 *     the rows it equals vr_hip_volume_histogram's output.
 * Out of scope: the device list (vr_hip_multi_*), a backdrop under a tf2d frame, labels together with a 2-D table, pre-integrated 2-D
 * classification, a shadow built from the 2-D table, MIP, isosurface, section and depth frames. */
#define VR_TF2D_ROWS_MAX 8
int vr_hip_set_tf2d(vr_ctx *ctx, const float *table, uint32_t rows, float g_scale, const uint32_t *esl_bits);   /* table NULL = drop */
int vr_hip_render_tf2d(vr_ctx *ctx, const vr_params *params, uint8_t *host_rgba);
int vr_hip_render_tf2d_device(vr_ctx *ctx, const vr_params *params, void *dev_rgba, void *stream);
int vr_hip_tf2d_frames(vr_ctx *ctx, uint64_t *frames_out);             /* testing aid: tf2d frames launched */
#define VR_GRADIENT_BINS_MAX 32
int vr_hip_gradient_histogram(vr_ctx *ctx, uint32_t g_bins, float g_scale, uint64_t *hist_out /* g_bins * 256 */, float *kernel_ms_out);

/* ---- fused frames: a second, co-registered field with a transfer function of its own.  No reference counterpart. ----
 * Two fields over the same grid in one frame — PET over CT, a dose or a flow inside anatomy, a temperature inside a density.  Each field
 * is classified by its own transfer function and the two are weighted against each other.  Compositing along a ray is not separable: the
 * second field's samples enter the same front-to-back accumulation at the same ray positions and the early termination is shared, so two
 * frames layered from outside do not give this frame.  A is the resident volume, B the second field.
 *  1. State.  B is context state beside the resident volume: dx * dy * dz voxels, x fastest, with the dims AND the bytes per voxel of the
 *     resident volume (other dims or another voxel size: VR_ERR_INVALID; no resident volume: VR_ERR_NOT_READY).  The bytes are copied; the
 *     host entry is synchronous, the device entry copies on the context's stream.  NULL drops B.  vr_hip_set_volume*, vr_hip_generate_volume
 *     drop it too: vr_hip_render_fused* then returns VR_ERR_NOT_READY.  B's transfer function is 128 premultiplied float4 in the layout
 *     vr_hip_set_transfer_fn takes; it is set together with 1024 ESL words, which are THE FUSED FRAME'S OWN leaping bits.  A bit means "block
 *     empty": the fused frame's bits are the AND of A's bits under A's function and B's bits under B's function; the caller builds them
 *     (vr_hip_set_tf2d's precedent: it takes the envelope's bits).  The call waits for the context's frames first, as
 *     vr_hip_set_transfer_fn does.  B's function and the bits survive a volume change until they are replaced.  Every other entry point
 *     ignores all of this; every existing struct keeps its size; the frames are counted by vr_hip_fused_frames (testing aid).  vr_fusion is
 *     given per call and is no state.
 *  2. Frame.  The composite frame vr_hip_render_device defines for a TRILINEAR or _Q8 frame under the context's clip (the identity clip when
 *     none is set, always run), gradient lighting and shadow.  The ray, clip_segment, leaping by params.esl on the fused bits, the k
 *     sequence, the band and crop partition and the pixel store are the labelled frame's.  (xb, yb, zb) = fma(k, A, B) are the sample's
 *     texel coordinates; steps 3-7 are one sample.
 *  3. Field A, unchanged.  cA is what the composite makes of A's sample: the filtered lookup, the `cA.w > 0.05f` test on the looked-up alpha,
 *     then the reference's cue or lighting steps 1-5, then the shadow's factor.  Nothing of A's arithmetic is new.
 *  4. Field B.  rawB is the interpolated value of B at the same coordinates with the same filter weights (rounded in _Q8); tbB is formed from
 *     rawB exactly as tb is formed from raw; cB is the filtered lookup in B's function.  B is emissive: no cue, no lighting, no shadow factor.
 *  5. Weights.  cA' = cA * weight_a and cB' = cB * weight_b, plain products on all four channels, formed behind step 3's shading.
 *  6. VR_FUSE_SUM.  Per channel c = fmaf(cB, weight_b, cA'); one accumulation acc = fmaf(c, 1 - acc.w, acc); then `acc.w > ray_threshold`.
 *  7. VR_FUSE_OVER.  A in front of B within the sample: acc = fmaf(cA', 1 - acc.w, acc); then, with the new acc.w,
 *     acc = fmaf(cB', 1 - acc.w, acc).  The termination test runs once, behind both.
 *  8. Exact acceleration.  A field's contribution is exactly 0 where its lookup is.  Its corner test and its tf_zero_below are derived from
 *     ITS OWN function exactly as vr_hip_set_transfer_fn derives them.  A wave may skip a field's unpacking and lookup when that field's test
 *     says so for every counting lane, and the whole sample only when both tests say so.  The cue, lighting and shadow fetches are needed
 *     for lanes dense in A alone.
 *  9. Consequences, each with equal leaping bits on both sides (or params.esl = 0).  (a) weight_b = 0 with any B, or B's function all zero,
 *     weight_a = 1 and A's own bits as the frame's bits, both modes: the bytes of vr_hip_render under the same state (x * 1 == x,
 *     fmaf(finite, 0, x) == x).  (b) weight_a = 0, weight_b = 1, no lighting, no shadow: the bytes of vr_hip_render with light_kd = 0 on a
 *     context whose resident volume is B, under B's function and the same bits.  (c) the special case of (b) one context shows: B a copy of
 *     A and B's function A's.  (d) Both weights 0, or both functions zero: all zero bytes.  (a)-(c) are NOT promised under the fused (AND)
 *     bits against a frame under one field's own bits: the single-field frame leaps blocks that are empty in its field alone, and a leap
 *     moves where the k sequence of the ray starts (k restarts at the leapt kx: other roundings behind it).  What holds with the AND bits: a
 *     field whose function is all zero has every bit set, so the AND is the other field's bits — (a) with B's function zero and (d) hold
 *     under the fused bits as well.
 *     In VR_FUSE_SUM, exchanging the two fields with their weights does NOT give the same accumulated values even without cue, lighting
 *     and shadow: fmaf(cB, wb, cA * wa) rounds cA * wa on its own and cB * wb not at all.  The difference is a rounding in the last bit of
 *     a float, so a byte of the frame differs only now and then.  The product and the fma are the contract; two fmas are not.
 * 10. Shadow.  The light grid is the context's, built from A under A's function (the label precedent).  B casts no shadow.
 * 11. Pre-integration.  VR_ERR_INVALID while vr_hip_set_preintegration(1) holds (the label precedent).
 * 12. What it reads.  A as a labelled frame reads it — the linear array, quad bricks or oct bricks: vr_launch_info::layout is 0, 1 or 5.  B is
 *     read in the same layout by the same kernel row: its base address is a kernel argument and A's staged address tables address it.  B's
 *     copy for the layout and chunk plane the frame chose is built from B's linear array on first use, on the context's stream and
 *     synchronous like any first use, while half of the HBM stays free; it is kept per kind and dropped with B.  Where the copy cannot be had
 *     the frame runs from both linear arrays (layout 0) instead of failing.  vr_hip_set_layout, vr_hip_set_wide_addressing and
 *     vr_hip_set_brick_plane apply.  Tiles start in grid order.  Frames are counted by vr_hip_timing and vr_hip_fused_frames and described
 *     by vr_hip_last_launch.
 * 13. Errors.  VR_ERR_INVALID for VR_SAMPLE_NEAREST, a NULL vr_fusion, mode > 1, reserved != 0, a weight that is not finite or lies outside
 *     [0, 1], a member of B's function that is negative or not finite, NULL bits with a function, and the dims or voxel-size mismatch.
 *     VR_ERR_NOT_READY without B or without B's function.  Everything else as for vr_hip_render*.
 * Out of scope: fields of differing dims, voxel size or registration; more than two fields; the device list (vr_hip_multi_*); a backdrop
 * under a fused frame; labels or a 2-D table together with fusion; B in MIP, isosurface, section and depth frames; a shadow cast by B;
 * volr_bench options and volr::HipRenderer. */
typedef struct vr_fusion {
	uint32_t mode;            /* VR_FUSE_SUM or VR_FUSE_OVER */
	float    weight_a;        /* 0..1: scales what field A contributes to a sample */
	float    weight_b;        /* 0..1: ... and field B */
	uint32_t reserved;        /* 0 */
} vr_fusion;                  /* 16 bytes; per call, not state */
#define VR_FUSE_SUM  0u
#define VR_FUSE_OVER 1u
int vr_hip_set_second_volume(vr_ctx *ctx, const void *host_voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t bytes_per_voxel);   /* NULL = drop */
int vr_hip_set_second_volume_device(vr_ctx *ctx, const void *dev_voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t bytes_per_voxel);
int vr_hip_set_second_transfer_fn(vr_ctx *ctx, const float *tf_premult_rgba, const uint32_t *fused_esl_bits);   /* waits for the context's frames first */
int vr_hip_render_fused(vr_ctx *ctx, const vr_params *params, const vr_fusion *fusion, uint8_t *host_rgba);
int vr_hip_render_fused_device(vr_ctx *ctx, const vr_params *params, const vr_fusion *fusion, void *dev_rgba, void *stream);
int vr_hip_fused_frames(vr_ctx *ctx, uint64_t *frames_out);            /* testing aid: fused frames launched */

/* What the last vr_hip_render* call of this context launched (tuning aid and test hook; no reference counterpart): the volume copy,
 * the lane order / wave shape / tile phase that were chosen (or forced), and the kernel's tile grid. */
typedef struct vr_launch_info {
	uint32_t layout;        /* 0 linear array, 1 quad bricks, 2 / 3 run bricks along z / y, 4 voxel bricks, 5 oct bricks, 6 both run copies (per tile),
	                           7 column windows (brick_plane then holds the march axis 0 x, 1 y, 2 z; column_voxels says which copy) */
	uint32_t brick_plane;   /* chunk plane of a quad copy: 0 (x,y), 1 (x,z), 2 (y,z) */
	uint32_t lane_map;      /* (lane order) + 4 * (wave shape), as in vr_hip_set_tile_mapping */
	uint32_t phase_x, phase_y;
	uint32_t clamp_fetch;   /* 1: the coordinate-clamping instantiation was needed */
	uint32_t tiles_x, tiles_y;
	uint32_t ordered;       /* 1: the frame ran in a measured-cost tile order */
	uint32_t straddle_permille;   /* orthogonal views along an axis: lane groups that still straddle cells under the chosen phase */
	uint32_t column_voxels; /* layout 7 with TRILINEAR: 1 = the march read the windows of 16 plain voxels (VR_COPY_COLV_*), 0 = the
	                           quad-element windows (VR_COPY_COL_*); vr_hip_set_column_copy */
	uint32_t column_shade_pairs; /* column_voxels = 1: 1 = the shading samples were fetched from the quad-element windows (one 8-byte load
	                           each), 0 = from the voxel windows (eight byte loads: unlit frames, mode 2, or that copy could not be had) */
	uint32_t shadowed;      /* 1: a shadowed composite frame (vr_hip_set_shadow; layout is then 0, 1 or 5) */
} vr_launch_info;
int vr_hip_last_launch(vr_ctx *ctx, vr_launch_info *out);

/* ---- timing: replaces the cudaEvent pair of Profiler.cpp:46-67 ---- */
int vr_hip_timing(vr_ctx *ctx, vr_timing *out);             /* synchronises the pending events */
int vr_hip_timing_reset(vr_ctx *ctx);

/* ---- feeders of the path on the GPU ----
 * Per-ESL-block min/max scan of RaycasterBase::set_volume (RaycasterBase.cpp:101-117) as an HBM-streaming reduction
 * over the resident volume.  minmax_out: 32*32*32 pairs {min,max} (uint8; u16 volumes use the high byte),
 * index z*1024 + y*32 + x; unused blocks keep {255, 0}.  esl_block_dims_out / esl_block_size_out follow
 * RaycasterBase.cpp:97-99,118-122.  kernel_ms_out (optional) = hipEvent time of the reduction kernel. */
int vr_hip_volume_minmax(vr_ctx *ctx, uint8_t *minmax_out, uint32_t *esl_block_dims_out, float *esl_block_size_out,
                         float *kernel_ms_out);
/* 256-bin histogram of the resident volume (ModelBase.cpp:19-33 raw counts; u16: high byte). */
int vr_hip_volume_histogram(vr_ctx *ctx, uint64_t *hist256_out, float *kernel_ms_out);

/* ---- synthetic benchmark volumes generated straight into HBM (SURVEY §8d "shell" / "noise") ----
 * kind 0 = shell, 1 = noise.  Replaces the resident volume (cube n^3). */
int vr_hip_generate_volume(vr_ctx *ctx, uint32_t kind, uint32_t n, uint32_t seed, uint32_t bytes_per_voxel);
/* copy the resident volume back (unpadded, x-fastest) — for checksums and for feeding the CPU baseline */
int vr_hip_download_volume(vr_ctx *ctx, void *host_out, uint64_t bytes);

/* ---- several MI355X behind one call (the reference drives one device, VolR.cpp:141-172) ----
 * One process, one context + stream per device, volume / TF / ESL replicated; a frame is cut into interleaved bands of rows
 * (band b -> devices[b mod n]), every device renders its bands, the RGBA8 bands travel to devices[0] over xGMI — RCCL
 * ncclSend / ncclRecv (communicators from ncclCommInitAll; librccl is loaded on demand) or peer copies when RCCL is not
 * available or a device is listed twice — and a copy kernel there de-interleaves them.  `params` describe the WHOLE frame
 * (partition fields are ignored); the image equals the single-device image byte for byte.
 * vr_hip_multi_render / _render_device are synchronous, like every renderer call of the reference.  _render_device_async queues
 * a frame and returns: up to three frames are in flight (band buffers, staging, events and per-device streams exist three times; nothing
 * is created per frame; the frames in flight must not share `dev_rgba`), frame i+1 renders while the bands of frame i travel; `consumer_stream` (hipStream_t on devices[0], may be NULL) is made to wait
 * for the assembled frame; vr_hip_multi_sync waits for everything queued.
 * A one-entry list is the single-device path.  The reference's `renderers[id]->render_volume()` reaches this through
 * volr::HipRenderer's device-list constructor (volume-rendering_amd/csrc/host/Renderer.h).
 * VERIFICATION STATE: with DISTINCT devices the RCCL / peer-copy transfer has not run on hardware yet (one-GPU build box); the
 * split, the gather by copies, the assemble kernel and the pipeline run with lists that repeat device 0, and the RCCL calls run
 * with VR_MULTI_TRANSPORT=rccl-self (one communicator, peer = self).  Therefore the first frame after every set_window on
 * distinct devices is self-checked on devices[0] (its own render of the other ranks' bands against what arrived; VR_ERR_HIP
 * "gather self-check failed" on a mismatch; VR_MULTI_SELFCHECK=0 disables, =1 forces it for any list). */
typedef struct vr_multi vr_multi;
int  vr_hip_multi_create(int n, const int *devices, vr_multi **out);
void vr_hip_multi_destroy(vr_multi *m);
const char *vr_hip_multi_last_error(const vr_multi *m);
int  vr_hip_multi_count(const vr_multi *m);
vr_ctx *vr_hip_multi_context(vr_multi *m, int rank);               /* the per-device context (feeders, layout knobs, timing) */
const char *vr_hip_multi_transport(const vr_multi *m);             /* "rccl" | "peer-copy" | "single" */
int  vr_hip_multi_set_window(vr_multi *m, uint32_t width, uint32_t height);
int  vr_hip_multi_set_transfer_fn(vr_multi *m, const float *tf_premult_rgba, const uint32_t *esl_bits);
int  vr_hip_multi_set_clip(vr_multi *m, const vr_clip *clip);      /* vr_hip_set_clip on every device's context */
int  vr_hip_multi_set_shadow(vr_multi *m, const vr_shadow *shadow); /* vr_hip_set_shadow on every device's context */
int  vr_hip_multi_set_lighting(vr_multi *m, const vr_lighting *lighting); /* vr_hip_set_lighting on every device's context */
int  vr_hip_multi_set_preintegration(vr_multi *m, uint32_t on);           /* vr_hip_set_preintegration on every device's context */
int  vr_hip_multi_set_volume(vr_multi *m, const void *host_voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t bytes_per_voxel);
int  vr_hip_multi_generate_volume(vr_multi *m, uint32_t kind, uint32_t n, uint32_t seed, uint32_t bytes_per_voxel);
int  vr_hip_multi_render(vr_multi *m, const vr_params *params, uint8_t *host_rgba);           /* whole frame -> host buffer */
int  vr_hip_multi_render_device(vr_multi *m, const vr_params *params, void *dev_rgba);        /* whole frame -> buffer on devices[0] */
int  vr_hip_multi_render_device_async(vr_multi *m, const vr_params *params, void *dev_rgba, void *consumer_stream);
int  vr_hip_multi_sync(vr_multi *m);
int  vr_hip_multi_prepare(vr_multi *m, uint32_t copies);                                      /* vr_hip_prepare on every device */
int  vr_hip_multi_timing(vr_multi *m, float *per_device_kernel_ms, float *total_ms);
/* the partition itself: frame row y belongs to device *rank_out and is row *local_row_out of that device's band buffer */
void vr_hip_multi_band_map(uint32_t n, uint32_t band_rows, uint32_t y, uint32_t *rank_out, uint32_t *local_row_out);
uint32_t vr_hip_multi_default_band_rows(uint32_t height, uint32_t n);

/* ---- brick copies: built lazily, or ahead of time ----
 * With VR_LAYOUT_BRICKED a frame reads one of up to six copies of the volume, chosen per frame from the sampling mode and the
 * view (volume-rendering_amd/csrc/vr_device.h).  set_volume only uploads the linear array; a copy is built (one kernel, 6-8 ms at
 * 1024^3, the context's stream, synchronous) by the first frame that wants it, so a NEAREST-only session holds the linear array
 * + the voxel bricks and nothing else.  vr_hip_prepare builds the copies named by `copies` (VR_COPY_* bits) now — what a
 * benchmark, or a caller about to vr_hip_release_linear_copy, does.  Copies the layout policy does not have at this volume
 * size (the second / third quad plane and the run bricks need 1-byte voxels and edges <= 1024; voxel bricks edges <= 2048; oct
 * bricks 2-byte voxels) are
 * skipped silently; every copy but the first quad copy is refused (VR_ERR_ALLOC) unless half of the HBM stays free — frames then
 * read the next best copy, see vr_volume_info::copies_refused.  No reference counterpart (GPURenderer4 builds its one cudaArray
 * in set_volume, GPURenderer4.cu:123-141). */
#define VR_COPY_QUAD_XY  (1u << 0)   /* quad bricks, 16-byte chunks in the (x,y) plane: TRILINEAR views along z (and every fallback) */
#define VR_COPY_QUAD_XZ  (1u << 1)   /* ... (x,z) plane: orthogonal views along y */
#define VR_COPY_QUAD_YZ  (1u << 2)   /* ... (y,z) plane: orthogonal views along x */
#define VR_COPY_RUN_Z    (1u << 3)   /* run bricks along z: TRILINEAR views that cannot be chunk-aligned, marching mostly along x or y */
#define VR_COPY_RUN_Y    (1u << 4)   /* run bricks along y: the same, marching mostly along z */
#define VR_COPY_VOXEL    (1u << 5)   /* voxel bricks: NEAREST */
#define VR_COPY_OCT      (1u << 6)   /* oct bricks (2-byte voxels only): one 16-byte element per cell = the whole 2x2x2 neighbourhood; what
                                        TRILINEAR reads for 2-byte voxels — one gather per sample instead of the quad bricks' two */
#define VR_COPY_COL_X    (1u << 7)   /* column windows along x / y / z (1-byte voxels, edges <= 2048): per cell column, four consecutive quad */
#define VR_COPY_COL_Y    (1u << 8)   /* elements along the axis in ONE aligned 16-byte word; what TRILINEAR reads for full-march frames of */
#define VR_COPY_COL_Z    (1u << 9)   /* ORTHOGONAL views along that axis: one gather and one transparency test per ~3 samples (vr_device.h) */
#define VR_COPY_COLV_X   (1u << 10)  /* the same for NEAREST: 16 consecutive VOXELS of a cell column in one aligned 16-byte word (1 byte per voxel): */
#define VR_COPY_COLV_Y   (1u << 11)  /* one gather and one transparency test per sixteen samples; TRILINEAR reads them too, and then shades from VR_COPY_COL_* (vr_hip_set_column_copy) */
#define VR_COPY_COLV_Z   (1u << 12)
#define VR_COPY_ALL      0x1fffu
#define VR_COPY_KINDS    13
/* Aligned run bricks along z / y (1-byte voxels, edges <= 1024): runs of 8 elements = 32 bytes that cover SEVEN cells, bricks of 2048 bytes —
 * no run straddles a 128-byte line, every line is one 2x2 block of cell columns (volume-rendering_amd/csrc/vr_device.h).  32/7 bytes per
 * voxel each.  Behind the VR_COPY_KINDS kinds and NOT part of VR_COPY_ALL, of vr_volume_info::copies_in_policy or ::build_ms:
 * built by the first full-march frame that reads them (vr_hip_set_run_flavour) or by vr_hip_prepare when their bit is named; resident or
 * refused they show under these bits in vr_volume_info::copies / ::copies_refused and count in ::bricked_bytes, their build times are in
 * vr_hip_run_aligned_info.
 * vr_hip_download_copy takes their bit indices 13 / 14. */
#define VR_COPY_RUN7_Z   (1u << 13)
#define VR_COPY_RUN7_Y   (1u << 14)
int vr_hip_prepare(vr_ctx *ctx, uint32_t copies);
/* Which flavour of the run bricks a frame reads that reads run bricks at all (vr_launch_info::layout 2, 3 or 6).
 *   0  automatic (the default): a FULL-MARCH frame (esl off, ray_threshold >= 1) reads the aligned kind (VR_COPY_RUN7_*) where it is
 *      resident or can be built, else the nine-element kind; every other frame — leaping, early termination — reads the nine-element kind;
 *   1  nine-element runs (VR_COPY_RUN_*) for every frame;
 *   2  seven-cell aligned runs for every full-march frame, as 0 (the switch exists for A/B runs and tests: 0 may stop choosing them).
 * The image is the same bit for bit whichever is read; which copy a tile reads, lane maps and wave shapes do not depend on it.  Anything
 * else is VR_ERR_INVALID.  Forgets nothing: the cached tile mappings do not depend on the flavour. */
int vr_hip_set_run_flavour(vr_ctx *ctx, uint32_t flavour);
/* The aligned run bricks of the resident volume and what the last composite frame read.  These facts live here and not in vr_volume_info /
 * vr_launch_info, whose sizes and members are pinned. */
typedef struct vr_run_aligned_info {
	uint32_t flavour;         /* vr_hip_set_run_flavour: 0, 1 or 2 */
	uint32_t last_flavour;    /* the last vr_hip_render* frame: 0 = it read no run bricks, 1 = nine-element runs, 2 = seven-cell aligned runs */
	uint32_t copies;          /* VR_COPY_RUN7_* bits resident now */
	uint32_t copies_refused;  /* VR_COPY_RUN7_* bits whose build was refused (HBM guard / allocation) */
	uint64_t bytes;           /* what the resident aligned copies occupy */
	float    build_ms[2];     /* hipEvent time of the kernel that built the copy along z / y (0 if never built) */
} vr_run_aligned_info;        /* 32 bytes */
int vr_hip_run_aligned_info(vr_ctx *ctx, vr_run_aligned_info *out);
/* Testing aid: the raw bytes of one resident brick copy (kind = bit index of its VR_COPY_* flag), so that a test can hold every copy
 * builder against a host-side construction of the layout, byte for byte.  *bytes_out (optional) = size of the copy; host_out may be
 * NULL for a size query.  VR_ERR_NOT_READY if the copy is not resident, VR_ERR_INVALID if capacity is too small. */
int vr_hip_download_copy(vr_ctx *ctx, uint32_t kind, void *host_out, uint64_t capacity, uint64_t *bytes_out);

/* ---- what the resident volume occupies in HBM, and giving some of it back ----
 * The bricked layout keeps the reference's linear array (feeders, download, building copies) next to the brick copies built so
 * far; every copy but the first is only built while at least half of the device memory stays free, so `brick_copies` may stay
 * smaller than `brick_copies_wanted` — a speed cliff this call makes visible (axis-aligned views along x / y then read the
 * (x,y) copy).  vr_hip_release_linear_copy frees the linear array once nothing will need it again: afterwards frames read the
 * copies that are resident (no further copy can be built: prepare first), while vr_hip_volume_minmax / _histogram /
 * vr_hip_download_volume / vr_hip_set_layout / vr_hip_set_wide_addressing(1) / vr_hip_prepare return VR_ERR_NOT_READY until the next set_volume (vr_hip_prepare: where it
 * would have to build a copy — naming only copies that are resident, or that the policy does not have, stays VR_OK), and so does a
 * frame that no resident copy can serve.  A second release is VR_OK.
 * Refused (VR_ERR_INVALID) when no brick copy is resident yet, for edges above 2048,
 * and while the index-arithmetic path is forced (vr_hip_set_wide_addressing 1). */
typedef struct vr_volume_info {
	uint32_t dim_x, dim_y, dim_z, bytes_per_voxel;
	uint32_t layout;                /* vr_layout actually in use */
	uint32_t brick_copies;          /* brick copies resident (0..3) */
	uint32_t brick_copies_wanted;   /* copies the layout policy asks for at this size (3: u8 with edges <= 1024, else 1; 0: linear) */
	uint32_t brick_planes;          /* bit i set = the copy with chunk plane i (0 (x,y), 1 (x,z), 2 (y,z)) is resident */
	uint32_t linear_resident;       /* 1 while the linear array is in HBM */
	uint32_t run_copy;              /* further copies resident: bit 0 run bricks along z, bit 1 run bricks along y (one 8-byte gather per
	                                   TRILINEAR sample), bit 2 voxel bricks (one voxel per element, what NEAREST reads) */
	uint64_t linear_bytes, bricked_bytes;
	uint32_t copies;                /* VR_COPY_* bits of the copies resident now */
	uint32_t copies_in_policy;      /* VR_COPY_* bits the layout policy has at this volume size (what frames may still build) */
	uint32_t copies_refused;        /* VR_COPY_* bits whose build was refused (HBM guard / allocation); not retried until vr_hip_prepare or set_volume */
	float    build_ms[VR_COPY_KINDS]; /* hipEvent time of the kernel that built copy i (0 if never built) */
	float    upload_ms;             /* wall time of the upload / generation of the linear array in the last set_volume */
} vr_volume_info;
int vr_hip_volume_info(vr_ctx *ctx, vr_volume_info *out);
int vr_hip_release_linear_copy(vr_ctx *ctx);

/* ---- introspection ---- */
int vr_hip_device_info(vr_ctx *ctx, char *name_out, size_t name_cap, uint32_t *compute_units, uint64_t *hbm_bytes);
const char *vr_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VR_HIP_H */
