// vr_fused.hip — fused composite frames (vr_hip_render_fused): the composite frame of a TRILINEAR view over TWO
// co-registered fields of the same dims and voxel size, each with a transfer function of its own and a weight against the other, accumulated
// in one front-to-back march with one early termination.  One kernel family, fused_kernel, over the 24 rows of the isosurface, and its launcher.
#include "vr_march.h"

namespace vr {

// LDS beside the brick tables: both premultiplied transfer functions with their per-entry deltas (the same fp32 subtraction the composite's
// dtf holds) and the ESL words of the fused frame.  12 KiB; with the 50 KiB of the 64-bit address tables a CU still holds two workgroups of
// 1024 threads, with the 17 KiB of the 32-bit ones four of 512: LDS never lowers the wave count.
struct __attribute__((aligned(16))) FusedTables {
	f4 tf[VR_TF_SIZE], dtf[VR_TF_SIZE];        // field A: the context's function
	f4 tfb[VR_TF_SIZE], dtfb[VR_TF_SIZE];      // field B: vr_hip_set_second_transfer_fn
	uint32_t esl[VR_ESL_VOLUME_SIZE];
};

// the kernel-argument segment of fused_kernel as a struct: its arguments in order
struct FusedKernelSegment { RayKernelArgs a; const void *vol; const float *tf; const uint32_t *esl; FusedArgs d; const float *tfb; uint32_t *out; };
typedef const FusedKernelSegment __attribute__((address_space(4))) *FusedSegment;

// the segment through the laundered kernel-argument pointer (vr_march.h clip_segment): what is read through it occupies no scalar register
// across the march
__device__ __forceinline__ FusedSegment fused_segment() {
	FusedSegment s = (FusedSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(s));
	return s;
}

// The reference's cue of a dense sample of field A (GPURenderer4.cu:41-51 shade_texture; the composite's, vr_raymarch_body.inc): the field a
// hundredth towards the light against the field here, scaled by light_kd — 0 where params.light_kd <= 0.01f.  Its constants through the
// laundered pointer.  Restated here as the label and tf2d units restate it.
template <int BPV, int ADDR, int LAYOUT, bool Q8>
__device__ __forceinline__ float fused_cue(const void *vol, const RayKernelArgs &ka, const uint32_t *lut, f3 p3, float xb, float yb, float zb, float raw) {
	const FusedSegment s = fused_segment();
	if (!(s->a.p.light_kd > 0.01f)) return 0.0f;                             // wave-uniform
	const f3 dl = mk3(s->a.p.view.light_pos[0] - p3.x, s->a.p.view.light_pos[1] - p3.y, s->a.p.view.light_pos[2] - p3.z);
	const float inv = rsqrt_nr(VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x)));
	const float qx = VR_FMA(dl.x * inv, s->a.lh_x, xb), qy = VR_FMA(dl.y * inv, s->a.lh_y, yb), qz = VR_FMA(dl.z * inv, s->a.lh_z, zb);
	const TriFetch<BPV, LAYOUT> lf = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, qx, qy, qz, true);
	const float raw_l = tri_resolve<BPV, LAYOUT, Q8>(lf, ka, qx, qy, qz);
	return (raw_l - raw) * s->a.kd_scaled;
}

// the filtered lookup of the composite in one of the two functions of the unit's tables
template <bool Q8>
__device__ __forceinline__ f4 fused_lookup(const f4 *tf, const f4 *dtf, float tb) {
	const uint32_t i = (uint32_t) (int) tb;
	const float w = filter_weight<Q8>(__builtin_amdgcn_fractf(tb));
	const f4 c0 = tf[i], dc = dtf[i];
	f4 col;
	col.x = VR_FMA(w, dc.x, c0.x); col.y = VR_FMA(w, dc.y, c0.y);
	col.z = VR_FMA(w, dc.z, c0.z); col.w = VR_FMA(w, dc.w, c0.w);
	return col;
}

// Per pixel: label_kernel's shape (vr_label.hip) — the ray of raymarch_kernel under clip_segment, leap_lane over this unit's ESL words (the
// fused frame's own: the caller's AND of both fields' bits), kBatch samples issued back to back before the first is consumed behind a
// sched_barrier, finished lanes composited with weight 0 — with TWO gathers per batch slot, field A's and field B's, at one set of texel
// coordinates: the row's address tables and index arithmetic address both copies, only the base differs.
//
// A sample: cA is what the composite makes of A's sample — the filtered lookup, the dense test, the cue or light_sample (wave-uniform:
// a.light_on), shadow_factor (a.shadow_on); cB is the filtered lookup of B's interpolated value in B's function, emissive: no cue, no
// lighting, no shadow.  cA' = cA * weight_a and cB' = cB * weight_b, plain products.  VR_FUSE_SUM: c = fma(cB, weight_b, cA'), one
// accumulation.  VR_FUSE_OVER: cA' accumulated, then cB' with the new acc.w.  One termination test behind both.  The mode is a
// wave-uniform word of the argument.
//
// Exact shortcuts, per wave and per field: (1) all corners of every counting lane below the field's skip_below, (2) the field's sample
// coordinate below its tf_zero_below — the field's lookup is exactly 0 for every counting lane, and 0 times a weight, fma(0, weight, x) and
// fma(0, t, acc) change nothing: its unpacking and lookup are skipped.  The whole sample is skipped only when both fields say so.
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void fused_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint32_t *__restrict__ esl_g,
                  const FusedArgs d, const float *__restrict__ tfb_g, uint32_t *out) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a fused frame is defined on the interpolated fields");
	// samples per batch: one on every row.  A slot holds two fetches, so a batch of one keeps as many loads in flight as label_kernel's two; at
	// two samples the rows of 1-byte voxels behind address tables need 65 registers, one more than 8 waves per SIMD allow, and every other
	// row 67-74 (DESIGN.md section 4.16 has the table of batch against registers)
#ifndef VR_FUSED_BATCH
	constexpr int kBatch = 1;
#else
	constexpr int kBatch = VR_FUSED_BATCH;
#endif
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	__shared__ FusedTables lds;
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	{
		const uint32_t t = threadIdx.x;
		if (t < 2u * VR_TF_SIZE) {                  // threads 0..127 stage A's function, 128..255 B's
			const bool second = t >= VR_TF_SIZE;
			const uint32_t e = second ? t - VR_TF_SIZE : t;
			const f4 *tf4 = (const f4 *) (second ? tfb_g : tf_g);
			const uint32_t e1 = e + 1 < VR_TF_SIZE ? e + 1 : VR_TF_SIZE - 1;
			const f4 c0 = tf4[e], c1 = tf4[e1];
			f4 dc;
			dc.x = c1.x - c0.x; dc.y = c1.y - c0.y; dc.z = c1.z - c0.z; dc.w = c1.w - c0.w;
			if (second) { lds.tfb[e] = c0; lds.dtfb[e] = dc; }
			else { lds.tf[e] = c0; lds.dtf[e] = dc; }
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
	const float threshold = a.p.ray_threshold;
	const void *volb = (const void *) (uintptr_t) d.vol_b;
	float k = kx;
	bool live = alive, done = false;
	f4 acc;
	acc.x = acc.y = acc.z = acc.w = 0.0f;
	while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
		TriFetch<BPV, LAYOUT> fa[kBatch], fb[kBatch];
		float ks[kBatch];
		bool counts[kBatch];
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			ks[u] = k;
			counts[u] = live;
			const float xb = VR_FMA(k, A.x, B.x), yb = VR_FMA(k, A.y, B.y), zb = VR_FMA(k, A.z, B.z);
			fa[u] = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, xb, yb, zb, true);
			fb[u] = tri_issue<BPV, ADDR, LAYOUT>(volb, a, lut, xb, yb, zb, true);      // the same cell, the same table entries: another base
			const float next = k + step;            // (a lane whose next sample lies beyond ky stays ON its last sample)
			live = live && next <= ky;
			k = live ? next : k;
		}
		__builtin_amdgcn_sched_barrier(0);
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			const bool c = counts[u] && !done;
			const uint32_t corners_a = fa[u].w0 | fa[u].w1 | fa[u].w2 | fa[u].w3;   // (words a layout does not fetch are 0)
			const uint32_t corners_b = fb[u].w0 | fb[u].w1 | fb[u].w2 | fb[u].w3;
			// (1), per field: skip_cmp is 0; a transfer function without leading zero entries comes with skip_mask 0 and skip_cmp 1: 0 != 1 always
			bool need_a = __builtin_amdgcn_ballot_w64(c && (corners_a & a.skip_mask) != a.skip_cmp) != 0ull;
			bool need_b;
			{
				const FusedSegment s = fused_segment();
				need_b = __builtin_amdgcn_ballot_w64(c && (corners_b & s->d.skip_mask_b) != s->d.skip_cmp_b) != 0ull;
			}
			if (!need_a && !need_b)
				continue;
			const float xb = VR_FMA(ks[u], A.x, B.x), yb = VR_FMA(ks[u], A.y, B.y), zb = VR_FMA(ks[u], A.z, B.z);
			f4 ca, cb;
			ca.x = ca.y = ca.z = ca.w = 0.0f;
			cb.x = cb.y = cb.z = cb.w = 0.0f;
			if (need_b) {                                                        // field B: emissive — its lookup and nothing else
				const float raw_b = tri_resolve<BPV, LAYOUT, kQ8>(fb[u], a, xb, yb, zb);
				const float tb_b = __builtin_amdgcn_fmed3f(VR_FMA(raw_b, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
				// (2)
				if (__builtin_amdgcn_ballot_w64(c && tb_b >= fused_segment()->d.tf_zero_below_b) != 0ull)
					cb = fused_lookup<kQ8>(lds.tfb, lds.dtfb, tb_b);
			}
			if (need_a) {                                                        // field A: the composite's sample, unchanged
				const float raw = tri_resolve<BPV, LAYOUT, kQ8>(fa[u], a, xb, yb, zb);
				const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
				// (2)
				if (__builtin_amdgcn_ballot_w64(c && tb >= a.tf_zero_below) != 0ull) {
					ca = fused_lookup<kQ8>(lds.tf, lds.dtf, tb);
					const uint64_t dense = __builtin_amdgcn_ballot_w64(c && ca.w > 0.05f);
					if (dense != 0ull) {
						if (fused_segment()->a.light_on != 0u) {                     // vr_hip_set_lighting: Blinn-Phong from A's gradient
							float m, spec;
							light_sample<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, A, B, origin, dir, ks[u], dense, ca.w, m, spec);
							ca.x = VR_FMA(ca.x, m, spec); ca.y = VR_FMA(ca.y, m, spec); ca.z = VR_FMA(ca.z, m, spec);
						} else {                                                     // the reference's cue; 0 for lanes that are not shaded
							const float diffuse = select_lanes(dense, fused_cue<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, march_point<SAMPLING>(origin, dir, ks[u]), xb, yb, zb, raw));
							ca.x += diffuse; ca.y += diffuse; ca.z += diffuse;
						}
						if (lit_frame_shadowed()) {                                  // vr_hip_set_shadow: the light grid of A's classification
							const float sf = select_lanes_else(dense, shadow_factor(march_point<SAMPLING>(origin, dir, ks[u])), 1.0f);
							ca.x *= sf; ca.y *= sf; ca.z *= sf;
						}
					}
				}
			}
			{   // steps 3-5: the weights and the mode, read here through the laundered pointer
				const FusedSegment s = fused_segment();
				const float wa = s->d.weight_a, wb = s->d.weight_b;
				ca.x = ca.x * wa; ca.y = ca.y * wa; ca.z = ca.z * wa; ca.w = ca.w * wa;
				const float t = c ? 1.0f - acc.w : 0.0f;                         // finished lanes: weight 0
				if (s->d.mode == VR_FUSE_SUM) {
					const float sx = VR_FMA(cb.x, wb, ca.x), sy = VR_FMA(cb.y, wb, ca.y), sz = VR_FMA(cb.z, wb, ca.z), sw = VR_FMA(cb.w, wb, ca.w);
					acc.x = VR_FMA(sx, t, acc.x); acc.y = VR_FMA(sy, t, acc.y);
					acc.z = VR_FMA(sz, t, acc.z); acc.w = VR_FMA(sw, t, acc.w);
				} else {                                                         // VR_FUSE_OVER: A in front of B within the sample
					acc.x = VR_FMA(ca.x, t, acc.x); acc.y = VR_FMA(ca.y, t, acc.y);
					acc.z = VR_FMA(ca.z, t, acc.z); acc.w = VR_FMA(ca.w, t, acc.w);
					const float t2 = c ? 1.0f - acc.w : 0.0f;
					cb.x = cb.x * wb; cb.y = cb.y * wb; cb.z = cb.z * wb; cb.w = cb.w * wb;
					acc.x = VR_FMA(cb.x, t2, acc.x); acc.y = VR_FMA(cb.y, t2, acc.y);
					acc.z = VR_FMA(cb.z, t2, acc.z); acc.w = VR_FMA(cb.w, t2, acc.w);
				}
			}
			done = done || (c && acc.w > threshold);                             // early ray termination, once, behind both fields
		}
		live = live && !done;
	}

	// -- write_color and the fused clear: a pixel without a sample has accumulated nothing and stores 0.  The output address is read again in
	// the kernel-argument segment here, behind the march, instead of kept across it
	const uint32_t rgba = map_float_int(acc.x, 256) | (map_float_int(acc.y, 256) << 8) | (map_float_int(acc.z, 256) << 16) | (map_float_int(acc.w, 256) << 24);
	fused_segment()->out[px] = rgba;
}

hipError_t launch_fused(const RayKernelArgs &args, const FusedArgs &fusion, const void *linear, const void *bricked, const void *second_linear,
                        const void *second_bricked, uint32_t bpv, const float *tf, const uint32_t *esl_bits, const float *second_tf,
                        void *out_rgba, hipStream_t stream) {
	if (second_linear == nullptr || second_tf == nullptr || esl_bits == nullptr || out_rgba == nullptr || (args.shadow_on && args.shadow_q == 0ull) ||
	    args.p.sampling == VR_SAMPLE_NEAREST || fusion.mode > VR_FUSE_OVER || (bricked != nullptr) != (second_bricked != nullptr))
		return hipErrorInvalidValue;
	// which of B's two arrays the row that will run reads: the one in the order of the array the row reads of A (the selector is the launcher's own)
	const bool reads_linear = select_variant(args, bricked != nullptr, bpv, [](auto, auto, auto, auto, bool linear_row) { return linear_row; });
	FusedArgs d = fusion;
	d.vol_b = (uint64_t) (uintptr_t) (reads_linear ? second_linear : second_bricked);
	RayKernelArgs a = args;
#ifdef VR_BOUNDS_CHECK
	// B's array is the second array the checks accept (bc_address): the rows of this family read no other alternate copy.  It has the size
	// of the array the row reads of A: the same dims, voxel size and order
	a.alt_copy = d.vol_b;
	a.bc_alt_bytes = a.bc_bytes;
#endif
	// the interpolated fields from the copies a MIP frame reads: never NEAREST (refused above), the run bricks or the voxel bricks
	return launch_tiles<rows_field>(a, linear, bricked, bpv, stream, NoDynamicLds(),
	                                [&](auto row) { return VR_ROW_KERNEL(fused_kernel, row); },
	                                tf, esl_bits, d, second_tf, (uint32_t *) out_rgba);
}

}  // namespace vr
