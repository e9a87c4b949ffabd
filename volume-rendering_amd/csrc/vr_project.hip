// vr_project.hip — the projections that keep one value per ray: maximum intensity (mip_kernel, mip_clipped, vr_mip_body.inc; the bounds
// they skip by) and the shaded isosurface (iso_kernel, iso_clipped, vr_iso_body.inc), with their launchers.
#include "vr_march.h"

namespace vr {

// ---- maximum-intensity projection (vr_hip_render_mip) ---------------------------------------------------------
//
// Per pixel: the ray of raymarch_kernel (get_ray, intersect), the sample sequence of its march with leaping off — k starts at kx, is
// accumulated by repeated addition of ray_step, every position is formed from k — and instead of a composite the running MAXIMUM m
// of the raw samples: NEAREST the integer voxel of Model::sample_data's unfused arithmetic, TRILINEAR the interpolated raw value
// (coordinates fma(k, A, B), the lerps of tri_resolve, Q8 weights rounded), m starting at 0.  The pixel is write_color of ONE
// transfer-function lookup of m (NEAREST transfer_fn[s8 / TF_RATIO], TRILINEAR the filtered lookup of a DVR sample), read from
// global memory once per ray: no table of it in LDS, no shading, no composite, no termination threshold.
//
// A sample is the march and the fetch.  kMipBatch samples are issued back to back before the first of them is consumed, so their
// gathers are in flight together (compiler-scheduled waits; every fetch clamps its cell like the reference, so any lane's address
// is in bounds whatever its k).  A lane fetches only while it is live AND needs the sample; a sample no lane needs issues nothing;
// the wave leaves when no lane is live.
//
// Exact acceleration (a.p.esl != 0).  m only grows, so a sample whose value cannot exceed m changes nothing:
//  * skipping: the bound of a sample is read from LDS by its ESL block index (block_index of the sample position: the grid of the
//    min/max scan).  NEAREST: the sample IS a voxel of that block, the bound is the block's maximum.  TRILINEAR: with v the voxel index
//    block_index forms per axis, the cell of the sample is floor(v - 1/2 +- rounding), i.e. v - 1 or v, its neighbour one more: the
//    eight corners lie within one voxel of the block, inside the 3x3x3 neighbouring blocks (edge >= 8 voxels) whose maximum is the
//    bound (the host keeps the frame out of this path when fp32 coordinates are not exact to a fraction of a cell: far-away views).
//    A lerp fma(t, b - a, a) with 0 <= t < 1 never leaves [min(a, b), max(a, b)], rounding included, so the interpolated value obeys
//    the bound too.  Q8 weights can round to exactly 1: the first two lerp levels are then still exact (1-byte voxels: all three —
//    every operand has at most 24 significant bits), the third may end one ulp above its larger operand for 2-byte voxels, which is
//    why that case compares against the next multiple of 256 (2-byte bounds are high bytes, padded with 0xff otherwise);
//  * stopping: once m has reached the volume's maximum the ray is finished (same bound, same argument).
// Both only skip fetches: k is advanced for every sample up to the point where the ray stops, so the image does not depend on them.
#ifndef VR_MIP_BATCH
#define VR_MIP_BATCH 4
#endif
constexpr int kMipBatch = VR_MIP_BATCH;
extern __shared__ __attribute__((aligned(16))) uint8_t mip_bound_lds[];      // kMipBoundEntries bytes of dynamic LDS, only for frames that skip

// mip_kernel and mip_clipped (a clipped frame: the segment narrowed by clip_segment) are one body, vr_mip_body.inc, compiled with CLIP = false / true
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void mip_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                uint32_t *__restrict__ out) {
	constexpr bool CLIP = false;
#include "vr_mip_body.inc"
}
// ... of a clipped frame (vr_hip_set_clip); a name of its own for the same reason as raymarch_clipped's
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void mip_clipped(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                 uint32_t *__restrict__ out) {
	constexpr bool CLIP = true;
#include "vr_mip_body.inc"
}

// block maxima of the min/max scan -> the MIP bounds (vr_device.h): one thread per block of the 32^3 grid
__global__ __launch_bounds__(256)
void mip_bounds_kernel(const uint8_t *__restrict__ minmax, uint8_t *__restrict__ bounds) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	constexpr int D = VR_ESL_VOLUME_DIMS;
	const int x = (int) (e % D), y = (int) ((e / D) % D), z = (int) (e / (D * D));
	uint32_t around = 0u;
	for (int dz = -1; dz <= 1; dz++)
		for (int dy = -1; dy <= 1; dy++)
			for (int dx = -1; dx <= 1; dx++) {
				const int nx = x + dx, ny = y + dy, nz = z + dz;
				if (nx < 0 || ny < 0 || nz < 0 || nx >= D || ny >= D || nz >= D) continue;
				const uint32_t v = minmax[2 * ((nz * D + ny) * D + nx) + 1];      // unused blocks hold 0 (minmax_init_kernel)
				around = v > around ? v : around;
			}
	const uint32_t own = minmax[2 * e + 1];
	bounds[e] = (uint8_t) own;
	bounds[kMipBoundEntries + e] = (uint8_t) around;
	if (own != 0u) atomicMax((uint32_t *) (bounds + 2u * kMipBoundEntries), own);
}

hipError_t launch_mip_bounds(const uint8_t *minmax_dev, uint8_t *bounds_dev, hipStream_t stream) {
	hipError_t e = hipMemsetAsync(bounds_dev + 2u * kMipBoundEntries, 0, kMipBoundBytes - 2u * kMipBoundEntries, stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(mip_bounds_kernel, dim3(kMipBoundEntries / 256u), dim3(256), 0, stream, minmax_dev, bounds_dev);
	return hipGetLastError();
}

hipError_t launch_mip(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf, const uint8_t *bounds,
                      void *out, hipStream_t stream) {
	if (args.p.esl != 0u && bounds == nullptr) return hipErrorInvalidValue;
	// a MIP frame never reads the run bricks (the caller does not ask for them); the bound table is dynamic LDS, so that frames which do
	// not skip keep every resident workgroup the address tables allow
	return launch_tiles<rows_no_run>(args, linear, bricked, bpv, stream,
	                                 [](auto, const RayKernelArgs &a) { return a.p.esl != 0u ? kMipBoundEntries : 0u; },
	                                 [&](auto row) { return args.clip_on ? VR_ROW_KERNEL(mip_clipped, row) : VR_ROW_KERNEL(mip_kernel, row); },
	                                 tf, bounds, (uint32_t *) out);
}

// ---- shaded isosurface with depth (vr_hip_render_iso) -----------------------------------------------------------
//
// Per pixel: the ray and the sample sequence of mip_kernel's TRILINEAR march, and instead of the maximum the FIRST sample whose
// interpolated raw value reaches `level`.  The march only looks for that sample: kMipBatch fetches issued back to back, consumed in order
// behind a sched_barrier, the first one at or above the level sets hi = its k and lo = the k of the sample before it (the last k of the
// previous batch when it is the batch's first), and ends the lane; the wave leaves when no lane is live.  Everything a hit costs beyond
// that runs AFTER the loop with the wave converged again — lanes hit at different samples, inside the loop it would run once per lane:
//  * `refine` bisection steps of [lo, hi] (wave-uniform trip count, one dependent fetch each; a lane without a hit, or one that hit
//    its first sample — lo == hi —, fetches its own hi again);
//  * six clamped fetches one texel either side of the surface point, issued together: central differences scaled by N/2 are the gradient
//    in model space; the pixel is the filtered transfer-function lookup of the level times fma(kd, |n . l|, 1 - kd);
//  * one store of the pixel and, where the caller gave a buffer, one of k* (or -1).
// Every fetch clamps its cell, so no lane can form an address outside its copy whatever its k.
//
// Exact acceleration (a.p.esl != 0).  A sample whose value is below the level cannot be the first hit, so its fetch may be skipped when
// its bound — the dilated block maximum mip_kernel skips by, widened the same way (argument there) — is below the level.  That is ONE
// bit per block: the workgroup builds the 1024-word table in LDS from the byte table build_mip_bounds keeps, 4 KiB instead of mip_kernel's
// 32 KiB, and reads it with the same block index.  k advances for every sample; bisection and gradient fetches are never skipped.
extern __shared__ __attribute__((aligned(16))) uint32_t iso_skip_lds[];      // VR_ESL_VOLUME_SIZE words of dynamic LDS, only for frames that skip

// iso_kernel and iso_clipped (a clipped frame: the segment narrowed by clip_segment — a hit at its first sample is the cut face, k* = the
// clipped kx, shaded from the field's gradient there) are one body, vr_iso_body.inc, compiled with CLIP = false / true
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void iso_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                const float level, const uint32_t refine, uint32_t *__restrict__ out, float *__restrict__ depth) {
	constexpr bool CLIP = false;
#include "vr_iso_body.inc"
}
// ... of a clipped frame (vr_hip_set_clip); a name of its own for the same reason as raymarch_clipped's
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void iso_clipped(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                 const float level, const uint32_t refine, uint32_t *__restrict__ out, float *__restrict__ depth) {
	constexpr bool CLIP = true;
#include "vr_iso_body.inc"
}

hipError_t launch_iso(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf, const uint8_t *bounds,
                      float level, uint32_t refine, void *out_rgba, void *out_depth, hipStream_t stream) {
	if (args.p.esl != 0u && bounds == nullptr) return hipErrorInvalidValue;
	// the interpolated field from the copies a MIP frame reads: never NEAREST (the caller refuses it), the run bricks or the voxel bricks;
	// the bit table is dynamic LDS: 4 KiB next to the address tables keep every resident workgroup frames without skipping have
	return launch_tiles<rows_field>(args, linear, bricked, bpv, stream,
	                                [](auto, const RayKernelArgs &a) { return a.p.esl != 0u ? VR_ESL_VOLUME_SIZE * 4u : 0u; },
	                                [&](auto row) { return args.clip_on ? VR_ROW_KERNEL(iso_clipped, row) : VR_ROW_KERNEL(iso_kernel, row); },
	                                tf, bounds, level, refine, (uint32_t *) out_rgba, (float *) out_depth);
}

}  // namespace vr
