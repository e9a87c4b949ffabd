// vr_depth.hip — depth frames of the composite and pixel picking (vr_hip_render_depth, vr_hip_pick): where along its
// ray the thing a composite pixel shows lies — the first sample at which the accumulated alpha reaches an opacity, the sample that contributes
// most, or the contribution-weighted mean —, the interpolated value there and the pixel's final alpha.  One kernel family, depth_kernel, over
// the 24 rows of the isosurface, its launcher, and the finishing kernel of a pick.
#include "vr_march.h"

namespace vr {

// LDS beside the brick tables: the alpha channel of the transfer function, its per-entry delta (the same fp32 subtraction the composite's
// dtf holds) and the alpha channel of the running integral K the host uploads behind the 128 entries; the ESL bits.
struct __attribute__((aligned(16))) DepthTables {
	float w[VR_TF_SIZE], dw[VR_TF_SIZE], kw[VR_TF_SIZE];
	uint32_t esl[VR_ESL_VOLUME_SIZE];
};

// the kernel-argument segment of depth_kernel as a struct: its arguments in order
struct DepthKernelSegment { RayKernelArgs a; const void *vol; const float *tf; const uint32_t *esl; DepthArgs d; float *depth, *value, *alpha; };

// Per pixel: the ray of raymarch_kernel (get_ray, intersect) under clip_segment (the identity clip when none is set), the composite's leaping
// loop in its plain per-lane form (vr_march.h leap_lane), and on what is left the composite's sample sequence — k starts at the leapt kx, advances by repeated
// addition of ray_step, every position is fma(k, A, B) — in the section kernel's shape: kBatch samples are issued back to back before the
// first is consumed behind a sched_barrier, in sample order.  Of the colour only the alpha channel is formed, with the composite's arithmetic:
// the filtered lookup, or the slab's narrow / wide forms (d.slab, wave-uniform).  A lane that is finished — beyond ky, or terminated by
// acc > ray_threshold inside a batch already issued — stays ON its last sample and fetches it again (every fetch clamps its cell: in bounds
// whatever k is); its alpha counts as 0, so g = 0 * t is 0, acc = fma(0, t, acc) is acc, and none of the three records moves: FIRST needs acc
// to change (opacity > 0), PEAK needs g > best >= 0, MEAN adds exact zeros.
//
// The mode is a wave-uniform kernel argument.  The three records share three registers: FIRST { found, k, raw }, PEAK { best, k, raw },
// MEAN { sg, sk, sv }.
//
// Exact shortcuts, per wave: (1) point classification: all corners of every counting lane below skip_below — the sample is transparent,
// nothing is unpacked; (2) the sample's coordinate and the slab's front both below tf_zero_below: alpha is exactly 0, no lookup.  A FIRST ray
// stops at its surface when no alpha buffer is asked for: depth and value are recorded by then.
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void depth_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint32_t *__restrict__ esl_g,
                  const DepthArgs d, float *depth, float *value, float *alpha) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a depth frame is defined on the interpolated field");
	// samples per batch: those of the section kernel of the same row, whose registers this kernel is held to
	constexpr int kBatch = BPV == 1 && ADDR == kAddrWide && LAYOUT == kLayoutBricked ? 3 : 4;
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	__shared__ DepthTables lds;
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	{
		const uint32_t t = threadIdx.x;
		if (t < VR_TF_SIZE) {
			const f4 *tf4 = (const f4 *) tf_g;
			const uint32_t t1 = t + 1 < VR_TF_SIZE ? t + 1 : VR_TF_SIZE - 1;
			const float w0 = tf4[t].w, w1 = tf4[t1].w;
			lds.w[t] = w0;
			lds.dw[t] = w1 - w0;
			lds.kw[t] = tf4[VR_TF_SIZE + t].w;
		}
		for (uint32_t i = t; i < VR_ESL_VOLUME_SIZE; i += kThreads) lds.esl[i] = esl_g[i];
	}
	__syncthreads();

	// -- tile = workgroup id: tiles start in grid order
	uint32_t tile_x, tile_y, lx, ly;
	tile_to_xy(a.tiles_x, a.tiles_y, blockIdx.x, blockIdx.x, tile_x, tile_y);
	lane_pixel<kThreads>(a, tile_x, tile_y, lx, ly);
	if (lx >= a.p.out_width || ly >= a.p.out_rows)
		return;                                     // no barrier below this point
	const size_t px = (size_t) ly * a.p.out_width + lx;

	const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
	f3 origin = ray.origin, dir = ray.dir;
	float kx = ray.kx, ky = ray.ky;
	const float step = a.p.ray_step;
	bool alive = clip_segment(origin, dir, kx, ky) && ray.alive;

	leap_lane<SAMPLING>(a, lds, origin, dir, kx, ky, alive);       // empty space leaping: the composite's loop, per lane (vr_march.h)
	alive = alive && (kx <= ky);                    // a fully empty ray is a miss
	if (!alive) { kx = 0.0f; ky = 0.0f; origin = mk3(0.0f, 0.0f, 0.0f); dir = origin; }      // lanes without a sample: position 0, never live

	// -- the march
	const f3 A = mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z);
	const f3 B = mk3(VR_FMA(origin.x, a.half_x, a.off_x), VR_FMA(origin.y, a.half_y, a.off_y), VR_FMA(origin.z, a.half_z, a.off_z));
	const uint32_t mode = d.mode;                   // wave-uniform: kernel arguments
	const bool slab = d.slab != 0u;
	const bool stop_at_surface = mode == VR_DEPTH_FIRST && d.want_alpha == 0u;
	const float threshold = a.p.ray_threshold;
	float k = kx;
	bool live = alive, done = false;
	float acc = 0.0f, tp = -1.0f;                   // tp: the clamped coordinate of the previous sample of this loop; below 0 = none yet
	float r0 = 0.0f, r1 = mode == VR_DEPTH_MEAN ? 0.0f : -1.0f, r2 = r1;
	while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
		TriFetch<BPV, LAYOUT> f[kBatch];
		float ks[kBatch];
		bool counts[kBatch];
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			ks[u] = k;
			counts[u] = live;
			f[u] = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z), true);
			const float next = k + step;            // (a lane whose next sample lies beyond ky stays ON its last sample)
			live = live && next <= ky;
			k = live ? next : k;
		}
		__builtin_amdgcn_sched_barrier(0);
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			const bool c = counts[u] && !done;
			const uint32_t corners = f[u].w0 | f[u].w1 | f[u].w2 | f[u].w3;     // (words a layout does not fetch are 0)
			// (1): skip_cmp is 0; a transfer function without leading zero entries comes with skip_mask 0 and skip_cmp 1: 0 != 1 always.
			// A slab frame resolves every sample: the next one needs this one's coordinate exactly
			if (!slab && __builtin_amdgcn_ballot_w64(c && (corners & a.skip_mask) != a.skip_cmp) == 0ull)
				continue;
			const float raw = tri_resolve<BPV, LAYOUT, kQ8>(f[u], a, VR_FMA(ks[u], A.x, B.x), VR_FMA(ks[u], A.y, B.y), VR_FMA(ks[u], A.z, B.z));
			const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
			const float tq = slab ? (tp < 0.0f ? tb : tp) : tb;                 // the front of the slab
			if (slab) tp = tb;
			// (2)
			if (__builtin_amdgcn_ballot_w64(c && (tb >= a.tf_zero_below || tq >= a.tf_zero_below)) == 0ull)
				continue;
			float aw;
			{
				const float tm = slab ? 0.5f * (tq + tb) : tb;                  // a narrow slab: the lookup at its middle
				const uint32_t i = (uint32_t) (int) tm;
				const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tm));
				aw = VR_FMA(w, lds.dw[i], lds.w[i]);
			}
			if (slab) {
				// a wide slab, |dt| >= 0.5: (K(tb) - K(tp)) / dt with full fp32 weights, the division, the difference and the product rounded once each
				const float dt = tb - tq;
				const bool wide = __builtin_fabsf(dt) >= 0.5f;
				if (__builtin_amdgcn_ballot_w64(c && wide) != 0ull) {
					auto integral = [&](float t) {
						const uint32_t i0 = (uint32_t) t, i = i0 < (uint32_t) (VR_TF_SIZE - 2) ? i0 : (uint32_t) (VR_TF_SIZE - 2);
						const float w = t - (float) i, hw = 0.5f * w;
						return VR_FMA(w, VR_FMA(hw, lds.dw[i], lds.w[i]), lds.kw[i]);
					};
					const float kp = integral(tq), kb = integral(tb);
					const float r = 1.0f / dt;
					aw = wide ? (kb - kp) * r : aw;
				}
			}
			aw = c ? aw : 0.0f;
			const float t = 1.0f - acc;
			const float g = aw * t;
			acc = VR_FMA(aw, t, acc);
			if (mode == VR_DEPTH_FIRST) {
				if (c && r0 == 0.0f && acc >= d.opacity) { r0 = 1.0f; r1 = ks[u]; r2 = raw; }
				if (stop_at_surface) done = done || r0 != 0.0f;
			} else if (mode == VR_DEPTH_PEAK) {
				if (g > r0) { r0 = g; r1 = ks[u]; r2 = raw; }
			} else {
				r0 = r0 + g; r1 = VR_FMA(ks[u], g, r1); r2 = VR_FMA(raw, g, r2);
			}
			done = done || (c && acc > threshold);  // early ray termination: the sample that terminates the ray is recorded above
		}
		live = live && !done;
	}

	// -- the result, and the fused clear: a pixel without a sample has recorded nothing and stores -1 / -1 / 0
	float out_k = r1, out_v = r2;
	if (mode == VR_DEPTH_MEAN) {
		const bool any = r0 > 0.0f;
		out_k = any ? r1 / r0 : -1.0f;
		out_v = any ? r2 / r0 : -1.0f;
	}
	// the three output addresses are read again in the kernel-argument segment here, behind the march, instead of kept across it (the rows
	// without address tables sit at the 80-SGPR limit of 8 waves per SIMD)
	typedef const DepthKernelSegment __attribute__((address_space(4))) *ConstSegment;
	ConstSegment seg = (ConstSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(seg));
	seg->depth[px] = out_k;
	if (seg->value != nullptr) seg->value[px] = out_v;      // (wave-uniform: kernel arguments)
	if (seg->alpha != nullptr) seg->alpha[px] = acc;
}

// One lane per query: the ray of the query's pixel formed again on the device, so position and voxel index carry the device's bits
__global__ __launch_bounds__(64)
void pick_finish_kernel(const RayKernelArgs a, uint32_t n, const uint32_t *__restrict__ xy, const float *__restrict__ depth,
                        const float *__restrict__ value, const float *__restrict__ alpha, vr_pick *__restrict__ out) {
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	if (i >= n) return;
	const PixelRay ray = pixel_ray(a, xy[2u * i], xy[2u * i + 1u]);
	const float k = depth[i];
	vr_pick r;
	r.hit = k >= 0.0f ? 1u : 0u;
	r.k = k; r.value = value[i]; r.alpha = alpha[i];
	r.position[0] = r.position[1] = r.position[2] = 0.0f;
	r.voxel[0] = r.voxel[1] = r.voxel[2] = 0.0f;
	if (r.hit) {
		const f3 pt = march_point<VR_SAMPLE_TRILINEAR>(ray.origin, ray.dir, k);
		const f3 A = mk3(ray.dir.x * a.half_x, ray.dir.y * a.half_y, ray.dir.z * a.half_z);
		const f3 B = mk3(VR_FMA(ray.origin.x, a.half_x, a.off_x), VR_FMA(ray.origin.y, a.half_y, a.off_y), VR_FMA(ray.origin.z, a.half_z, a.off_z));
		r.position[0] = pt.x; r.position[1] = pt.y; r.position[2] = pt.z;
		r.voxel[0] = VR_FMA(k, A.x, B.x); r.voxel[1] = VR_FMA(k, A.y, B.y); r.voxel[2] = VR_FMA(k, A.z, B.z);
	} else {
		r.k = -1.0f; r.value = -1.0f;
	}
	out[i] = r;
}

hipError_t launch_depth(const RayKernelArgs &args, const DepthArgs &depth, const void *linear, const void *bricked, uint32_t bpv,
                        const float *tf, const uint32_t *esl_bits, void *out_depth, void *out_value, void *out_alpha, hipStream_t stream) {
	if (depth.mode > VR_DEPTH_MEAN || out_depth == nullptr || esl_bits == nullptr) return hipErrorInvalidValue;
	// the interpolated field from the copies a MIP frame reads: never NEAREST (the caller refuses it), the run bricks or the voxel bricks
	return launch_tiles<rows_field>(args, linear, bricked, bpv, stream, NoDynamicLds(),
	                                [&](auto row) { return VR_ROW_KERNEL(depth_kernel, row); },
	                                tf, esl_bits, depth, (float *) out_depth, (float *) out_value, (float *) out_alpha);
}

hipError_t launch_pick_finish(const RayKernelArgs &a, uint32_t n, const uint32_t *xy, const float *depth, const float *value, const float *alpha,
                              vr_pick *out, hipStream_t stream) {
	if (n == 0u) return hipSuccess;
	hipLaunchKernelGGL(pick_finish_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, a, n, xy, depth, value, alpha, out);
	return hipGetLastError();
}

}  // namespace vr
